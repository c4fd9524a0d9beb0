"""CTC prefix beam search with a label language model or a lexicon fused in, host side (no GPU): the library and the package carry
the feature; the numpy twin that DEFINES what klstm_ctc_beam_decode_lm computes (tests/ctc_beam_lm_ref.py) is the LM-less twin
where the LM is trivial, and is held to independent float64 statements (the textbook dictionary-keyed search with the same factors,
the exact label probability times the weights along the labelling); the table builders of kaldi-lstm_amd/lm.py; forbidden
extensions; and that a matching bigram lowers the error count on ambiguous posteriors."""
import itertools
import json
import math
import os

import numpy as np
import pytest

from tests import cpp_driver
from tests import ctc_beam_lm_ref as L
from tests import ctc_beam_ref as Bm
from tests.ctc_decode_ref import levenshtein
from tests.test_ctc_beam import GRID_SEEDS, all_prefixes, exhaustive_case, grid_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGINS = os.path.join(ROOT, "profiles", "ctc_beam_lm_parity_margins.json")


def build_ctc_beam_lm_driver():
    return cpp_driver.build("ctc_beam_lm_test")


def run_driver(*args):
    return cpp_driver.run("ctc_beam_lm_test", *args)


def margin(name):
    """the bar of a float64 comparison: 10 x the largest deviation the NUMPY TWIN shows on the same inputs (profiles/README.md)"""
    with open(MARGINS) as fh:
        return json.load(fh)[name]["bar"]


# ---------------------------------------------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------------------------------------------
def trivial_lm(K):
    return np.zeros((1, K), np.int32), np.ones((1, K), np.float32), None


def bigram_next(K):
    """Q = K + 1: state 1 + c after label c"""
    return np.tile(1 + np.arange(K, dtype=np.int32), (K + 1, 1))


def grid_bigram(seed, K, final=False):
    """the bigram of the issue for grid_case(seed): rows from Dirichlet(0.3), alpha = 0.7, beta = 0.5 folded in, on even seeds 20 % of
    the entries zeroed"""
    rng = np.random.RandomState(7000 + seed)
    p = rng.dirichlet([0.3] * K, size=K + 1)
    wt = (p ** 0.7 * math.exp(0.5)).astype(np.float32)
    if seed % 2 == 0:
        wt[rng.rand(K + 1, K) < 0.2] = 0.0
    fin = (0.05 + rng.rand(K + 1)).astype(np.float32) if final else None
    return bigram_next(K), wt, fin


def random_trigram(rng, K, zero=0.2, final=True):
    """Q = 1 + K + K^2 states with random weights around 1, a share of them 0"""
    import kaldi_lstm_amd as k
    nxt = k.lm.ngram_next(K, 3)
    wt = np.exp(rng.randn(*nxt.shape)).astype(np.float32)
    wt[rng.rand(*nxt.shape) < zero] = 0.0
    return nxt, wt, ((0.05 + rng.rand(nxt.shape[0])).astype(np.float32) if final else None)


_GRID = {}


def grid_lm_result(seed):
    """the LM twin's full beam (N = B) on grid_case(seed) with grid_bigram(seed), computed once"""
    if seed not in _GRID:
        y, K, T, B, C = grid_case(seed)
        lm = grid_bigram(seed, K)
        _GRID[seed] = (y, B, lm, L.beam_twin_lm(y, [T], 0, B, C, B, lm))
    return _GRID[seed]


# ---------------------------------------------------------------------------------------------------------------------------------
# the feature exists (fails on a tree without it)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_library_and_package_carry_the_language_model():
    import inspect
    import kaldi_lstm_amd as k
    lib = k.load_library()
    assert hasattr(lib, "klstm_ctc_beam_decode_lm") and hasattr(lib, "klstm_ctc_beam_lm_resident")
    assert "lm" in inspect.signature(k.ctc_beam_decode).parameters
    assert inspect.isclass(k.CtcLabelLm) and callable(k.ngram_label_lm) and callable(k.lexicon_label_lm)
    with open(os.path.join(ROOT, "include", "klstm_nnet.hpp")) as fh:
        hpp = fh.read()
    assert "class CtcLabelLm" in hpp and "SetLanguageModel" in hpp


# ---------------------------------------------------------------------------------------------------------------------------------
# the twin against the LM-less twin and against float64
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", GRID_SEEDS)
def test_trivial_lm_is_the_search_without_one(seed):
    """Q = 1, every weight 1: the same prefixes, the same pb / pnb BITS, the same exponent"""
    y, K, T, B, C = grid_case(seed)
    e = Bm.emissions(y[:, 0])
    nxt, wt, _ = L.lm_tables(trivial_lm(K))
    a, Ea = Bm.beam_stream(e, 0, B, C)
    b, Eb = L.beam_stream_lm(e, 0, B, C, nxt, wt)
    assert Ea == Eb and len(a) == len(b)
    for (pa, pba, pnba), (pb_, pbb, pnbb, q) in zip(a, b):
        assert pa == pb_ and q == 0
        assert np.float32(pba).view(np.int32) == np.float32(pbb).view(np.int32)
        assert np.float32(pnba).view(np.int32) == np.float32(pnbb).view(np.int32)


# the twin extends by the `cands` best classes of a frame, the textbook search by every class: at K = 48 (cands = 32 < K - 1) a class
# of low emission and high LM weight can enter the textbook beam only.  Seed 7 (K = 48, T = 40, peaked) is that case.
TEXTBOOK_EXCEPTIONS = {7: "K = 48, cands = 32: the textbook search extends by a class outside the 32 candidates"}


def test_twin_one_best_equals_the_textbook_search_with_the_same_factors():
    worst, differs, changed = 0.0, [], 0
    for seed in GRID_SEEDS:
        y, B, lm, tw = grid_lm_result(seed)
        assert tw["score"][0][0] > -np.inf, seed                                   # no utterance is dead
        tb = L.textbook_lm64(Bm.emissions64(y[:, 0]), 0, B, lm)
        if tuple(tw["hyp"][0][0]) != tb[0][0]:
            differs.append(seed)
            continue
        worst = max(worst, abs(float(tw["score"][0][0]) - tb[0][1]) / abs(tb[0][1]))
        _, K, T, _, C = grid_case(seed)
        changed += tw["hyp"][0][0] != Bm.beam_twin(y, [T], 0, B, C, 1)["hyp"][0][0]
    print("1-best differs from the textbook search on seeds", differs, "; largest relative score deviation on the others:", worst,
          "; the LM changed the 1-best on", changed, "of 40")
    assert len(differs) <= 2 and set(differs) <= set(TEXTBOOK_EXCEPTIONS)
    assert changed == 35                                                           # inputs and twin are deterministic; the test can tell an LM from none
    assert worst <= margin("textbook_rel")


def test_exhaustive_beam_gives_exact_fused_probabilities():
    """K = 3, T <= 5, B = 64, C = 2: nothing is pruned, so every listed score is log p(labels | y) + the log weights along the labels
    (+ log final), with and without final weights"""
    worst = 0.0
    for final in (False, True):
        for seed, T in enumerate((1, 2, 3, 4, 5, 5, 5, 5)):
            y = exhaustive_case(seed, T)
            rng = np.random.RandomState(900 + seed)
            lm = (bigram_next(3), np.exp(rng.randn(4, 3)).astype(np.float32), (0.1 + rng.rand(4)).astype(np.float32) if final else None)
            if seed % 2:
                lm[1][rng.randint(4), 1 + rng.randint(2)] = 0.0
            tw = L.beam_twin_lm(y, [T], 0, 64, 2, 64, lm)
            e64 = Bm.emissions64(y[:, 0])
            exact = {tuple(p): Bm.label_logp64(e64, 0, p) + L.lm_logw64(lm, p) for p in all_prefixes(T)}
            exact = {p: v for p, v in exact.items() if v > -np.inf}
            assert tw["nbest_count"][0] == len(exact) and {tuple(h) for h in tw["hyp"][0]} == set(exact)
            for h, sc in zip(tw["hyp"][0], tw["score"][0]):
                worst = max(worst, abs(float(sc) - exact[tuple(h)]) / abs(exact[tuple(h)]))
    print("largest relative deviation of the exhaustive LM twin from the exact fused log p:", worst)
    assert worst <= margin("exhaustive_rel")


@pytest.mark.parametrize("final", [False, True])
def test_lists_hold_no_duplicate_and_scores_descend(final):
    for seed in GRID_SEEDS:
        y, K, T, B, C = grid_case(seed)
        tw = grid_lm_result(seed)[3] if not final else L.beam_twin_lm(y, [T], 0, B, C, B, grid_bigram(seed, K, final=True))
        hy = [tuple(h) for h in tw["hyp"][0]]
        assert len(set(hy)) == len(hy) == tw["nbest_count"][0] <= B, seed
        sc = [float(v) for v in tw["score"][0]]
        assert sc == sorted(sc, reverse=True), seed


def test_final_weights_reorder_and_drop():
    y, K, T, B, C = grid_case(4)
    nxt, wt, _ = grid_bigram(4, K)
    base = L.beam_twin_lm(y, [T], 0, B, C, B, (nxt, wt, None))
    fin = np.ones(K + 1, np.float32)
    drop = base["state"][0][0]
    fin[drop] = 0.0                                              # the best hypothesis ends in a state that may not end
    tw = L.beam_twin_lm(y, [T], 0, B, C, B, (nxt, wt, fin))
    kept = [h for h, q in zip(base["hyp"][0], base["state"][0]) if q != drop]
    assert tw["hyp"][0] == kept and drop not in tw["state"][0]
    dead = L.beam_twin_lm(y, [T], 0, B, C, B, (nxt, wt, np.zeros(K + 1, np.float32)))
    assert dead["nbest_count"] == [1] and dead["score"][0] == [-np.inf] and dead["hyp"][0] == base["hyp"][0][:1]


# ---------------------------------------------------------------------------------------------------------------------------------
# the table builders
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2, 3])
def test_ngram_rows_sum_to_one(order):
    import kaldi_lstm_amd as k
    rng = np.random.RandomState(order)
    K, blank = 6, 2
    labels = [c for c in range(K) if c != blank]
    seqs = [[labels[i] for i in rng.randint(0, K - 1, rng.randint(0, 9))] for _ in range(50)]
    nxt, wt, fin = k.ngram_label_lm(seqs, K, blank, order=order, add_k=0.5, alpha=1.0, beta=0.0)
    Q = (1, 1 + K, 1 + K + K * K)[order - 1]
    assert nxt.shape == wt.shape == (Q, K) and fin.shape == (Q,) and nxt.dtype == np.int32 and wt.dtype == np.float32
    assert np.all(wt[:, blank] == 0) and np.all((nxt >= 0) & (nxt < Q))
    np.testing.assert_allclose(wt.astype(np.float64).sum(1) + fin, 1.0, rtol=1e-6)
    # the states are the histories: the automaton scores a sequence as the n-gram does
    seq = seqs[3] + [labels[0]]
    hist = ([], seq[-1:], seq[-2:])[order - 1]
    assert L.lm_walk(nxt, seq) == L.lm_walk(nxt, hist)
    # alpha and beta are folded in
    n2, w2, f2 = k.ngram_label_lm(seqs, K, blank, order=order, add_k=0.5, alpha=0.7, beta=0.5)
    np.testing.assert_allclose(w2, wt.astype(np.float64) ** 0.7 * math.exp(0.5), rtol=1e-6)
    np.testing.assert_allclose(f2, fin.astype(np.float64) ** 0.7, rtol=1e-6)


def test_lexicon_accepts_exactly_the_word_sequences():
    """tf > 0 iff the hypothesis is a separator-joined sequence of words: checked on every labelling of up to 6 labels"""
    import kaldi_lstm_amd as k
    K, blank, sep = 5, 0, 4
    words = [[1, 2], [1, 2, 3], [3], [2, 1]]
    lm = k.lexicon_label_lm(words, K, blank, sep)
    accepted = set()
    for n in range(1, 4):
        for ws in itertools.product(words, repeat=n):
            seq = list(ws[0])
            for w in ws[1:]:
                seq += [sep] + list(w)
            accepted.add(tuple(seq))
    for n in range(7):
        for p in itertools.product(range(1, K), repeat=n):
            assert (L.lm_logw64(lm, p) > -np.inf) == (p in accepted), p
    # through the search: everything the twin lists is a word sequence
    rng = np.random.RandomState(21)
    z = rng.randn(12, 1, K)
    y = (np.exp(z) / np.exp(z).sum(-1, keepdims=True)).astype(np.float32)
    tw = L.beam_twin_lm(y, [12], blank, 16, 4, 16, lm)
    assert tw["score"][0][0] > -np.inf
    for h in tw["hyp"][0]:
        assert L.lm_logw64(lm, h) > -np.inf, h


# ---------------------------------------------------------------------------------------------------------------------------------
# forbidden extensions
# ---------------------------------------------------------------------------------------------------------------------------------
def has_transition(nxt_tab, hyp, q, c):
    s = 0
    for x in hyp:
        if s == q and x == c:
            return True
        s = int(nxt_tab[s, x])
    return False


def forbidden_case(seed):
    """grid_case(seed) with its bigram, a tenth of the transitions forbidden by weight 0 and a tenth by a next outside [0, Q)"""
    y, K, T, B, C = grid_case(seed)
    nxt, wt, _ = grid_bigram(seed, K)
    rng = np.random.RandomState(8000 + seed)
    wt = np.where(wt == 0, np.float32(0.3), wt)
    zero = rng.rand(K + 1, K) < 0.1
    bad = (rng.rand(K + 1, K) < 0.1) & ~zero
    wt[zero] = 0.0
    nx = nxt.copy()
    nx[bad] = rng.choice([-1, -7, K + 1, K + 50, 2 ** 31 - 1, -2 ** 31], size=int(bad.sum()))
    return y, K, T, B, C, nxt, (nx, wt, None), zero | bad


def test_forbidden_transitions_are_absent():
    seen = 0
    for seed in GRID_SEEDS[:12]:
        y, K, T, B, C, nxt, lm, forb = forbidden_case(seed)
        tw = L.beam_twin_lm(y, [T], 0, B, C, B, lm)
        free = L.beam_twin_lm(y, [T], 0, B, C, B, (nxt, np.where(lm[1] == 0, np.float32(0.3), lm[1]), None))
        for q, c in zip(*np.nonzero(forb[:, 1:])):
            assert not any(has_transition(nxt, h, q, c + 1) for h in tw["hyp"][0]), (seed, q, c + 1)
            seen += any(has_transition(nxt, h, q, c + 1) for h in free["hyp"][0])
    assert seen > 0                                              # without the zeros the lists do hold such transitions


def test_an_utterance_whose_every_path_is_forbidden_is_dead():
    y, K, T, B, C = grid_case(3)
    nxt, wt, _ = grid_bigram(3, K)
    y = y.copy()
    y[5, 0, 0] = 0.0                                              # frame 5 has no blank: a label must be emitted ...
    for lm in ((nxt, np.zeros_like(wt), None), (np.full_like(nxt, -1), wt, None)):     # ... and none may
        tw = L.beam_twin_lm(y, [T], 0, B, C, B, lm)
        assert tw["nbest_count"] == [1] and tw["score"][0] == [-np.inf]


# ---------------------------------------------------------------------------------------------------------------------------------
# the LM helps: sequences of a sparse Markov chain, rendered with ambiguous frames
# ---------------------------------------------------------------------------------------------------------------------------------
def markov_case(seed, K=9, n_tokens=8, frames_per_token=3):
    """-> (y [T, 1, K], reference).  Label a is followed by one of two labels only.  Every token is a run of frames_per_token frames and
    a blank frame; in every third token the true label shares its frames with a rival the chain forbids there, the rival slightly
    ahead: the acoustic evidence alone picks the rival."""
    rng = np.random.RandomState(seed)
    succ = {a: (1 + a % (K - 1), 1 + (a + 2) % (K - 1)) for a in range(1, K)}
    ref = [1 + rng.randint(K - 1)]
    while len(ref) < n_tokens:
        ref.append(succ[ref[-1]][rng.randint(2)])
    rows = []
    for j, c in enumerate(ref):
        for _ in range(frames_per_token):
            p = np.full(K, 0.02, np.float32)
            if j % 3 == 1:
                rival = next(r for r in range(1, K) if r != c and r not in succ[ref[j - 1]])
                p[c], p[rival] = 0.38, 0.44
            else:
                p[c] = 0.8
            rows.append(p / p.sum())
        p = np.full(K, 0.02, np.float32)
        p[0] = 0.8
        rows.append(p / p.sum())
    return np.asarray(rows, np.float32)[:, None, :], ref, succ


def test_a_matching_bigram_lowers_the_error_count():
    import kaldi_lstm_amd as k
    K = 9
    rng = np.random.RandomState(77)
    _, _, succ = markov_case(0, K)
    train = []
    for _ in range(400):
        seq = [1 + rng.randint(K - 1)]
        while len(seq) < 8:
            seq.append(succ[seq[-1]][rng.randint(2)])
        train.append(seq)
    lm = k.ngram_label_lm(train, K, 0, order=2, add_k=0.01)
    with_lm = without = 0
    for u in range(32):
        y, ref, _ = markov_case(100 + u, K)
        T = y.shape[0]
        without += levenshtein(Bm.beam_twin(y, [T], 0, 8, 4, 1)["hyp"][0][0], ref)
        with_lm += levenshtein(L.beam_twin_lm(y, [T], 0, 8, 4, 1, lm)["hyp"][0][0], ref)
    print("1-best edit errors over 32 utterances: without an LM", without, ", with the matching bigram", with_lm)
    assert with_lm < without


# ---------------------------------------------------------------------------------------------------------------------------------
# the C-ABI's host-side answers
# ---------------------------------------------------------------------------------------------------------------------------------
def test_lm_limits_and_plan_query():
    import kaldi_lstm_amd as k
    lib = k.load_library()
    n = None

    def call(Q, K, nxt=None, wt=None):
        return lib.klstm_ctc_beam_decode_lm(n, 10, 4, K, K, n, 0, n, 4, 4, 1, Q, nxt, wt, n, n, n, n, n, n, n, n, n, n, 0, n)
    assert call((1 << 24) // 8 + 1, 8) == 2                       # states * K beyond 2^24: refused before any pointer is looked at
    assert call(0, 8) == 2 and call(-3, 8) == 2                   # 1 <= states
    assert call((1 << 24) // 8, 8) == 1                           # the limit itself: the null pointers are next
    assert lib.klstm_ctc_beam_lm_resident(1, 8, 4, 4) == 1        # a table of 64 bytes fits
    assert lib.klstm_ctc_beam_lm_resident(1 << 20, 16, 4, 4) == 0
    assert lib.klstm_ctc_beam_lm_resident(0, 16, 4, 4) == 0 and lib.klstm_ctc_beam_lm_resident((1 << 24) // 8 + 1, 8, 4, 4) == 0
    # the answer flips exactly once as the table grows
    flips = [lib.klstm_ctc_beam_lm_resident(q, 64, 16, 8) for q in range(1, 4200, 7)]
    assert flips == sorted(flips, reverse=True)
