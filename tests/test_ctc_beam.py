"""CTC prefix beam search, host side (no GPU): the library and the package carry the feature, the numpy twin that DEFINES what
klstm_ctc_beam_decode computes (tests/ctc_beam_ref.py) is checked against independent float64 statements (the textbook
dictionary-keyed search, the exact label probability of the forward recurrence), and the host-side answers of the C-ABI."""
import itertools
import json
import os

import numpy as np
import pytest

from tests import cpp_driver
from tests import ctc_beam_ref as Bm
from tests import ctc_decode_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGINS = os.path.join(ROOT, "profiles", "ctc_beam_parity_margins.json")


def build_ctc_beam_driver():
    return cpp_driver.build("ctc_beam_test")


def run_driver(*args, ok=True):
    return cpp_driver.run("ctc_beam_test", *args, ok=ok)


def margin(name):
    """the bar of a float64 comparison: 10 x the largest deviation the NUMPY TWIN shows on the same inputs (profiles/README.md)"""
    with open(MARGINS) as fh:
        return json.load(fh)[name]["bar"]


# ---------------------------------------------------------------------------------------------------------------------------------
# the inputs: the grid of the issue.  K in {5, 12, 29, 48}, T in {20, 40, 60, 80}, B in {4, 8, 16}, C = min(K - 1, 32); even seeds are
# random softmax rows, odd seeds peaked_case of tests/ctc_decode_ref.py with one edit of every kind.  No seed had to be swapped out.
# ---------------------------------------------------------------------------------------------------------------------------------
GRID_SEEDS = list(range(40))


def softmax_rows(rng, T, S, K, scale=2.0):
    z = rng.randn(T, S, K) * scale
    y = np.exp(z - z.max(-1, keepdims=True))
    return (y / y.sum(-1, keepdims=True)).astype(np.float32)


def grid_case(seed):
    """-> (y [T, 1, K], K, T, B, C)"""
    K, T, B = (5, 12, 29, 48)[seed % 4], (20, 40, 60, 80)[(seed // 4) % 4], (4, 8, 16)[seed % 3]
    rng = np.random.RandomState(1000 + seed)
    if seed % 2 == 0:
        y = softmax_rows(rng, T, 1, K)
    else:
        ref = rng.randint(1, K, max(1, T // 4)).tolist()
        y = D.peaked_case(seed, T, K, 0, [ref], [T], [(1, 1, 1, 1)])
    return y, K, T, B, min(K - 1, 32)


_GRID = {}


def grid_result(seed):
    """the twin's full beam (N = B) on grid_case(seed), computed once"""
    if seed not in _GRID:
        y, K, T, B, C = grid_case(seed)
        _GRID[seed] = (y, B, Bm.beam_twin(y, [T], 0, B, C, B))
    return _GRID[seed]


def score_excess(y, tw, s=0, n=None):
    """largest (score - exact log p(hyp | y)) / |exact| over the list of stream s: the search sums a SUBSET of the alignments of a
    labelling, so only rounding can lift its score above the exact value"""
    e64 = Bm.emissions64(y[:n, s] if n else y[:, s])
    worst = -np.inf
    for h, sc in zip(tw["hyp"][s], tw["score"][s]):
        ex = Bm.label_logp64(e64, 0, h)
        worst = max(worst, (float(sc) - ex) / abs(ex))
    return worst


def exhaustive_case(seed, T):
    rng = np.random.RandomState(500 + seed)
    return softmax_rows(rng, T, 1, 3, scale=1.5)


def all_prefixes(T):
    return [list(p) for n in range(T + 1) for p in itertools.product((1, 2), repeat=n)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the feature exists (fails on a tree without it)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_library_and_package_carry_the_beam_decoder():
    import kaldi_lstm_amd as k
    lib = k.load_library()
    assert hasattr(lib, "klstm_ctc_beam_decode") and hasattr(lib, "klstm_ctc_beam_workspace_bytes")
    assert callable(k.ctc_beam_decode) and callable(k.nbest_to_lists) and callable(k.ctc_beam_workspace_bytes)


# ---------------------------------------------------------------------------------------------------------------------------------
# the twin against independent statements
# ---------------------------------------------------------------------------------------------------------------------------------
def test_hash_is_the_spelled_out_one():
    assert Bm.prefix_hash([]) == 0x243F6A8885A308D3
    x = ((0x243F6A8885A308D3 ^ 4) * 0x9E3779B97F4A7C15) % 2 ** 64
    assert Bm.prefix_hash([3]) == x ^ (x >> 29)
    seen = {Bm.prefix_hash(p) for p in all_prefixes(5)}
    assert len(seen) == 63


@pytest.mark.parametrize("seed", GRID_SEEDS)
def test_twin_one_best_equals_the_textbook_search(seed):
    y, B, tw = grid_result(seed)
    tb = Bm.textbook64(Bm.emissions64(y[:, 0]), 0, B)
    assert tuple(tw["hyp"][0][0]) == tb[0][0]
    assert abs(float(tw["score"][0][0]) - tb[0][1]) <= 1e-5 * abs(tb[0][1])        # the same sum: float32 chain against float64 chain


def test_twin_lists_hold_no_duplicate():
    for seed in GRID_SEEDS:
        _, B, tw = grid_result(seed)
        hy = [tuple(h) for h in tw["hyp"][0]]
        assert len(set(hy)) == len(hy) == tw["nbest_count"][0] <= B, seed
        sc = [float(v) for v in tw["score"][0]]
        assert sc == sorted(sc, reverse=True), seed


def test_twin_score_is_a_lower_bound_of_the_exact_label_probability():
    """measured on the twin (profiles/ctc_beam_parity_margins.json): the largest relative excess is 3.8e-8, a float32 rounding"""
    worst = max(score_excess(grid_result(seed)[0], grid_result(seed)[2]) for seed in GRID_SEEDS)
    print("largest relative excess of the twin's score over the exact log p:", worst)
    assert worst <= margin("lower_bound_rel")


def test_exhaustive_beam_gives_exact_label_probabilities():
    """T <= 5, K = 3, B = 64, C = 2: all 63 prefixes fit, nothing is pruned, so every score IS log p(labels | y).  Measured on the twin:
    largest relative deviation 4.3e-7"""
    worst = 0.0
    for seed, T in enumerate((1, 2, 3, 4, 5, 5, 5, 5)):
        y = exhaustive_case(seed, T)
        tw = Bm.beam_twin(y, [T], 0, 64, 2, 64)
        e64 = Bm.emissions64(y[:, 0])
        exact = {tuple(p): Bm.label_logp64(e64, 0, p) for p in all_prefixes(T)}
        exact = {p: v for p, v in exact.items() if v > -np.inf}          # a labelling with repeats needs a blank between them
        assert tw["nbest_count"][0] == len(exact) and {tuple(h) for h in tw["hyp"][0]} == set(exact)
        for h, sc in zip(tw["hyp"][0], tw["score"][0]):
            worst = max(worst, abs(float(sc) - exact[tuple(h)]) / abs(exact[tuple(h)]))
        order = sorted(exact.items(), key=lambda it: -it[1])[:tw["nbest_count"][0]]
        got = [exact[tuple(h)] for h in tw["hyp"][0]]
        # ordered by the exact probability (up to the rounding of the float32 totals the twin sorts by)
        assert all(a >= b - 1e-6 * abs(b) for a, b in zip(got, got[1:]))
        assert abs(got[0] - order[0][1]) <= 1e-6 * abs(order[0][1])
    print("largest relative deviation of the exhaustive twin from the exact log p:", worst)
    assert worst <= margin("exhaustive_rel")


def test_twin_emissions_candidates_and_ties():
    y = np.array([[0.1, 0.4, 0.4, 0.05, 0.05], [np.nan, 2.0 ** -61, np.inf, -np.inf, 2.0 ** -60]], np.float32)
    e = Bm.emissions(y)
    assert e[1].tolist() == [0.0, 0.0, 2.0 ** 60, 0.0, 2.0 ** -60]
    assert Bm.candidates(e[0], 0, 3) == [1, 2, 3]              # equal emissions: the lower column first
    assert Bm.candidates(e[0], 1, 2) == [2, 0]
    assert Bm.candidates(e[1], 0, 4) == [2, 4]                 # only e > 0 counts
    w = np.array([1.0, 2.0, 4.0, 1.0, 1.0], np.float32)        # equal PRODUCTS from different y and w
    yy = np.array([0.5, 0.25, 0.125, 0.0, 0.0], np.float32)
    assert Bm.candidates(Bm.emissions(yy, w), 4, 3) == [0, 1, 2]


def test_twin_statuses_totals_and_dead_utterance():
    rng = np.random.RandomState(3)
    y = softmax_rows(rng, 12, 6, 7)
    y[4, 5] = np.nan                                            # stream 5 dies in frame 4
    lens = [12, 0, 9, 12, 13, 12]
    refs = [[1, 2, 3], [1], [], [1, 8, 2], [1], [2, 2]]
    tw = Bm.beam_twin(y, lens, 0, 4, 3, 3, refs=refs)
    assert tw["nbest_count"][1] == 0 and tw["nbest_count"][4] == 0 and tw["errors"][1] == [-1] * 3 and tw["errors"][4] == [-1] * 3
    assert tw["errors"][3] == [-1] * 3 and tw["nbest_count"][3] == 3          # label 8 outside [0, K): the list yes, errors no
    assert tw["errors"][2][0] == len(tw["hyp"][2][0])                        # empty reference
    assert tw["nbest_count"][5] == 1 and tw["score"][5] == [-np.inf]          # dead: the first entry alone
    counted = (0, 2, 5)
    assert tw["totals"] == [sum(tw["errors"][s][0] for s in counted), 5, sum(len(tw["hyp"][s][0]) for s in counted), 3,
                            sum(tw["errors"][s][0] > 0 for s in counted), sum(min(tw["errors"][s][:tw["nbest_count"][s]]) for s in counted)]
    assert tw["totals"][5] <= tw["totals"][0]


def test_beam_one_with_one_candidate_follows_the_frame_winners():
    """B = 1, C = 1 on peaked posteriors: the single prefix is the collapsed best path"""
    refs = [[1, 2, 2, 3, 1], [4, 4, 4]]
    lens = [40, 30]
    y = D.peaked_case(5, 40, 9, 0, refs, lens, [(0, 0, 0, 0), (1, 0, 0, 0)])
    tw = Bm.beam_twin(y, lens, 0, 1, 1, 1, refs=refs)
    g = D.decode_twin(y, lens, 0, refs=refs)
    assert [h[0] for h in tw["hyp"]] == g["hyp"]


# ---------------------------------------------------------------------------------------------------------------------------------
# the C-ABI's host-side answers
# ---------------------------------------------------------------------------------------------------------------------------------
def test_beam_workspace_query_and_limits():
    import kaldi_lstm_amd as k
    lib = k.load_library()
    a, b = k.ctc_beam_workspace_bytes(1000, 16, 16, 8), k.ctc_beam_workspace_bytes(2000, 16, 16, 8)
    assert 1000 * 16 * 8 * (8 + 16) <= a <= 1000 * 16 * 8 * (8 + 16) + 8192 and a < b
    assert k.ctc_beam_workspace_bytes(65535, 1, 64, 32) < 64 << 20
    for T, S, B, C in ((2048, 32, 4, 4), (1, 33, 4, 4), (65536, 1, 4, 4), (0, 1, 4, 4), (10, 4, 65, 4), (10, 4, 0, 4), (10, 4, 4, 33),
                       (10, 4, 4, 0)):
        with pytest.raises(k.KlstmError) as ei:
            k.ctc_beam_workspace_bytes(T, S, B, C)
        assert ei.value.status == 2 and b"klstm_ctc_beam_workspace_bytes" in lib.klstm_last_error()
    # refused before anything touches the device: sizes first, then pointers
    n = None

    def call(T, S, K, B, C, N):
        return lib.klstm_ctc_beam_decode(n, T, S, K, K, n, 0, n, B, C, N, n, n, n, n, n, n, n, n, n, 0, n)
    assert call(10, 33, 8, 4, 4, 1) == 2 and call(2048, 32, 8, 4, 4, 1) == 2
    assert call(10, 4, 40000, 4, 4, 1) == 2 and call(10, 4, 1, 4, 1, 1) == 2
    assert call(10, 4, 8, 65, 4, 1) == 2 and call(10, 4, 64, 4, 33, 1) == 2
    assert call(10, 4, 8, 4, 8, 1) == 2                          # candidates beyond K - 1
    assert call(10, 4, 8, 4, 4, 5) == 2                          # n-best beyond the beam
    assert call(10, 4, 8, 0, 4, 1) == 1 and call(10, 4, 8, 4, 0, 1) == 1 and call(10, 4, 8, 4, 4, 0) == 1
    assert call(10, 4, 8, 64, 7, 64) == 1                        # every limit met: the null pointers are next
