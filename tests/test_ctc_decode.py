"""CTC best-path decoding, host side (no GPU): the library and the package carry the feature, the numpy twin that DEFINES what
klstm_ctc_decode computes (tests/ctc_decode_ref.py) is checked against independent statements, the host-side answers of the C-ABI, and
the reordering of DecodeCtcWholeUtterances (include/klstm_nnet.hpp) into utterance order through tests/cpp/ctc_decode_test."""
import itertools

import numpy as np
import pytest

from tests import cpp_driver
from tests import ctc_decode_ref as D
from tests import ctc_ref as R
from tests.test_ctc import plain_utts



def build_ctc_decode_driver():
    return cpp_driver.build("ctc_decode_test")


def run_driver(*args, ok=True):
    return cpp_driver.run("ctc_decode_test", *args, ok=ok)


# ---------------------------------------------------------------------------------------------------------------------------------
# the feature exists (fails on a tree without it)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_library_and_package_carry_the_decoder():
    import kaldi_lstm_amd as k
    lib = k.load_library()
    assert hasattr(lib, "klstm_ctc_decode") and hasattr(lib, "klstm_ctc_decode_workspace_bytes")
    assert callable(k.ctc_greedy_decode) and callable(k.hypotheses_to_lists)


# ---------------------------------------------------------------------------------------------------------------------------------
# the twin against independent statements
# ---------------------------------------------------------------------------------------------------------------------------------
def test_collapse_equals_groupby():
    rng = np.random.RandomState(0)
    for blank in (0, 2, 4):
        for n in (0, 1, 2, 7, 50, 400):
            path = rng.randint(0, 5, n) if n < 400 else np.repeat(rng.randint(0, 5, 80), 5)
            want = [c for c, _ in itertools.groupby(path.tolist()) if c != blank]
            assert D.collapse(path, blank) == want


def _lev_rec(a, b):
    if not a:
        return len(b)
    if not b:
        return len(a)
    return min(_lev_rec(a[1:], b) + 1, _lev_rec(a, b[1:]) + 1, _lev_rec(a[1:], b[1:]) + (a[0] != b[0]))


def test_levenshtein_equals_exhaustive_recursion():
    seqs = [list(p) for n in range(5) for p in itertools.product(range(3), repeat=n)]
    assert len(seqs) == 121
    for a in seqs:
        for b in seqs:
            assert D.levenshtein(a, b) == _lev_rec(tuple(a), tuple(b))


def test_levenshtein_is_a_metric_on_random_sequences():
    rng = np.random.RandomState(1)
    for _ in range(60):
        a, b, c = (rng.randint(0, 4, rng.randint(0, 40)).tolist() for _ in range(3))
        ab, ba = D.levenshtein(a, b), D.levenshtein(b, a)
        assert ab == ba and (ab == 0) == (a == b)
        assert abs(len(a) - len(b)) <= ab <= max(len(a), len(b))
        assert D.levenshtein(a, c) <= ab + D.levenshtein(b, c)


def test_frame_classes_keys_ties_nan_and_weights():
    y = np.zeros((6, 1, 5), np.float32)
    y[0, 0] = [0.1, 0.4, 0.4, 0.05, 0.05]               # tie: the lowest column
    y[1, 0] = [np.nan, 0.2, np.nan, 0.3, 0.1]            # a NaN never wins
    y[2, 0] = np.nan                                     # nothing but NaN: column 0
    y[3, 0] = [0.1, np.inf, 0.2, np.inf, 0.3]            # +inf wins, lowest first
    y[4, 0] = 0.0                                        # all equal: column 0
    y[5, 0] = [0.5, 0.25, 0.125, 0.0, 0.0]
    assert D.frame_classes(y, [6])[:, 0].tolist() == [1, 3, 0, 1, 0, 0]
    w = np.array([1.0, 2.0, 4.0, 1.0, 1.0], np.float32)  # equal PRODUCTS from different y and w: 0.5, 0.5, 0.5
    assert D.frame_classes(y, [6], w)[5, 0] == 0
    w[0] = 0.5
    assert D.frame_classes(y, [6], w)[5, 0] == 1
    assert D.frame_classes(y, [4])[4:, 0].tolist() == [-1, -1]          # padding
    assert (D.frame_classes(y, [0]) == -1).all() and (D.frame_classes(y, [7]) == -1).all()


def test_twin_statuses_and_totals():
    y, _ = R.make_case(2, 30, 8, 3.0, [30, 0, 25, 30, 31], [0] * 5)
    y = y.numpy()
    refs = [[1, 2, 3], [1], [], [1, 8, 2], [1]]
    tw = D.decode_twin(y, [30, 0, 25, 30, 31], 0, refs=refs)
    assert tw["hyp"][1] == [] and tw["hyp"][4] == [] and tw["errors"][1] == -1 and tw["errors"][4] == -1
    assert tw["errors"][3] == -1 and len(tw["hyp"][3]) > 0                      # label 8 outside [0, K): hypothesis yes, errors no
    assert tw["errors"][2] == len(tw["hyp"][2])                                 # empty reference
    assert tw["totals"] == [tw["errors"][0] + tw["errors"][2], 3, len(tw["hyp"][0]) + len(tw["hyp"][2]), 2,
                            (tw["errors"][0] > 0) + (tw["errors"][2] > 0)]
    assert (tw["frame_class"][:, 1] == -1).all() and (tw["frame_class"][25:, 2] == -1).all()


def test_peaked_case_covers_small_distances():
    refs = [[1, 2, 2, 3, 1], [4, 4, 4], [1, 2, 3, 4, 5, 6, 7], [2]]
    lens = [60, 40, 55, 9]
    corrupt = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 1, 1), (0, 0, 2, 0)]
    y = D.peaked_case(5, 60, 9, 0, refs, lens, corrupt)
    tw = D.decode_twin(y, lens, 0, refs=refs)
    assert tw["errors"][0] == 0 and tw["hyp"][0] == refs[0]
    assert all(0 <= e <= 4 for e in tw["errors"]) and sum(tw["errors"]) > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# the C-ABI's host-side answers
# ---------------------------------------------------------------------------------------------------------------------------------
def test_decode_workspace_query_and_limits():
    import kaldi_lstm_amd as k
    lib = k.load_library()
    a, b = k.ctc_decode_workspace_bytes(1000, 16, 150), k.ctc_decode_workspace_bytes(2000, 16, 150)
    assert 2 * 1000 * 16 * 4 <= a <= 2 * 1000 * 16 * 4 + 4096 and a < b
    assert k.ctc_decode_workspace_bytes(65535, 1, 1023) < 1 << 20
    for T, S, L in ((2048, 32, 0), (1, 33, 0), (65536, 1, 0), (0, 1, 0), (10, 4, 1024), (10, 4, -1)):
        with pytest.raises(k.KlstmError) as ei:
            k.ctc_decode_workspace_bytes(T, S, L)
        assert ei.value.status == 2 and b"klstm_ctc_decode_workspace_bytes" in lib.klstm_last_error()
    # refused before anything touches the device: sizes first, then pointers
    n = None
    assert lib.klstm_ctc_decode(n, 10, 33, 8, 8, n, 0, n, n, n, n, n, n, n, n, n, n, 0, n) == 2
    assert lib.klstm_ctc_decode(n, 10, 4, 40000, 40000, n, 0, n, n, n, n, n, n, n, n, n, n, 0, n) == 2
    assert lib.klstm_ctc_decode(n, 10, 4, 1, 1, n, 0, n, n, n, n, n, n, n, n, n, n, 0, n) == 2
    assert lib.klstm_ctc_decode(n, 10, 4, 8, 8, n, 0, n, n, n, n, n, n, n, n, n, n, 0, n) == 1


# ---------------------------------------------------------------------------------------------------------------------------------
# DecodeCtcWholeUtterances hands results back in the order of the utterance list
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,sort,max_frames,lens", [
    (3, 1, 0, [5, 9, 0, 7, 9, 2, 30000]),            # the 30000-frame utterance and the empty one are skipped: empty results
    (4, 0, 8, [5, 9, 3, 7, 9, 2, 8, 1, 6]),          # list order, two over the cap, one stream idle in the last minibatch
    (4, 1, 0, [6, 6, 2, 6, 9, 2, 6, 2]),             # ties keep the order of the list
    (1, 1, 0, [3, 1, 2]),
    (8, 1, 0, [4, 2]),
])
def test_results_come_back_in_utterance_order(S, sort, max_frames, lens):
    r = run_driver("order", S, sort, max_frames, ",".join(str(v) for v in lens))
    lines = r.stdout.split("\n")
    got = [[int(v) for v in ln.split(",")] if ln else [] for ln in lines[1:1 + len(lens)]]
    cap = max_frames if max_frames > 0 else 65535 // S
    utts = plain_utts(lens)
    batches, skipped = R.batch_twin(utts, S, bool(sort), cap)
    want = [[] for _ in lens]
    for mb in batches:                                   # what each stream of the twin's minibatches carries, by utterance number
        for s, i in enumerate(mb["index"]):
            if i >= 0:
                want[i] = [mb["lens"][s], int(mb["feat"][s, 0])] + mb["labels"][s]
    assert int(lines[0].split()[1]) == skipped == sum(1 for w in want if not w)
    assert got == want
    for i, n in enumerate(lens):
        assert want[i] == ([] if not 0 < n <= cap else [n, 1000 * i] + utts[i][1])
