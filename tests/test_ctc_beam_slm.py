"""Sparse back-off language models for the CTC beam search, host side (no GPU): the library and the package carry the feature; the ARPA
reader against a dense table computed independently from the file's probabilities; the count-based builder sums to 1; the twin
(tests/ctc_beam_slm_ref.py) gives the same lists from the expansion and from lazy tables; the seeds of the back-off coverage test
meet its condition; the host mirror of the device's validation; the C++ reader writes the arrays of the Python reader."""
import math
import os

import numpy as np
import pytest

from tests import cpp_driver
from tests import ctc_beam_ref as Bm
from tests import ctc_beam_slm_ref as R
from tests.test_ctc_beam import softmax_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_ctc_beam_slm_driver():
    return cpp_driver.build("ctc_beam_slm_test")


def run_driver(*args):
    return cpp_driver.run("ctc_beam_slm_test", *args)


# ---------------------------------------------------------------------------------------------------------------------------------
# the feature exists (fails on a tree without it)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_library_and_package_carry_the_sparse_model():
    import inspect
    import kaldi_lstm_amd as k
    lib = k.load_library()
    for name in ("klstm_ctc_slm_bytes", "klstm_ctc_slm_build", "klstm_ctc_beam_decode_slm", "klstm_ctc_beam_stream_step_slm"):
        assert hasattr(lib, name), name
    assert inspect.isclass(k.CtcSparseLabelLm)
    for fn in (k.sparse_lm_lookup, k.sparse_lm_to_dense, k.arpa_label_lm, k.backoff_ngram_label_lm):
        assert callable(fn)
    with open(os.path.join(ROOT, "include", "klstm_nnet.hpp")) as fh:
        hpp = fh.read()
    assert "class CtcSparseLabelLm" in hpp and "ReadArpaLabelLm" in hpp and "CtcSparseLabelLm *slm" in hpp


def test_size_query_and_its_limits():
    import kaldi_lstm_amd as k
    lib = k.load_library()
    assert lib.klstm_ctc_slm_bytes(100, 1000, 64) >= 100 * 16 + 1000 * 44
    for states, arcs, K in ((0, 10, 8), ((1 << 24) + 1, 10, 8), (10, 0, 8), (10, (1 << 26) + 1, 8), (10, 10, 1), (10, 10, 32769)):
        assert lib.klstm_ctc_slm_bytes(states, arcs, K) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# the ARPA reader: a hand-written file of order 3 over six symbols, one token that maps to no class
# ---------------------------------------------------------------------------------------------------------------------------------
ARPA_SYMBOLS = {"a": 1, "b": 2, "c": 3, "d": 4, "e": 5, "f": 6}
ARPA_K, ARPA_BLANK = 7, 0
ARPA_GRAMS = {
    1: [(-99.0, "<s>", -0.40), (-1.00, "</s>", None), (-0.90, "a", -0.30), (-0.95, "b", -0.25), (-1.10, "c", -0.35), (-1.20, "d", -0.20),
        (-1.30, "e", -0.15), (-1.40, "f", None), (-1.50, "zz", -0.10)],
    2: [(-0.40, "<s> a", -0.20), (-0.70, "<s> c", None), (-0.30, "a b", -0.45), (-1.10, "a </s>", None), (-0.50, "b c", -0.22),
        (-0.80, "b zz", -0.10), (-0.60, "c a", None), (-0.35, "d e", -0.31), (-0.45, "e f", None), (-0.55, "f </s>", None),
        (-0.65, "c c", -0.12)],
    3: [(-0.20, "<s> a b", None), (-0.25, "a b c", None), (-0.90, "a b </s>", None), (-0.33, "b c a", None), (-0.15, "d e f", None),
        (-0.42, "c c c", None), (-0.10, "zz a b", None)],
}


def arpa_text():
    out = ["\\data\\"] + ["ngram %d=%d" % (n, len(g)) for n, g in ARPA_GRAMS.items()] + [""]
    for n, grams in ARPA_GRAMS.items():
        out.append("\\%d-grams:" % n)
        out += ["%.2f\t%s" % (lp, words) + ("\t%.2f" % bow if bow is not None else "") for lp, words, bow in grams]
        out.append("")
    return "\n".join(out + ["\\end\\", ""])


def arpa_tables():
    """the file's probabilities as dictionaries over tuples of classes (-1: <s>, -2: </s>), the grams with `zz` left out"""
    tok = dict(ARPA_SYMBOLS, **{"<s>": -1, "</s>": -2})
    logp, logbow = {}, {}
    for grams in ARPA_GRAMS.values():
        for lp, words, bow in grams:
            if "zz" in words.split():
                continue
            g = tuple(tok[w] for w in words.split())
            logp[g] = lp
            if bow is not None:
                logbow[g] = bow
    return logp, logbow


def backed_off_log10(logp, logbow, h, w):
    """log10 P(w | h) as the ARPA format defines it, in float64"""
    acc = 0.0
    while True:
        if h + (w,) in logp:
            return acc + logp[h + (w,)]
        if not h:
            return -math.inf
        acc += logbow.get(h, 0.0)
        h = h[1:]


@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (0.9, 0.2)])
def test_arpa_expansion_equals_an_independent_dense_table(alpha, beta):
    import kaldi_lstm_amd as k
    model = k.arpa_label_lm(arpa_text(), ARPA_SYMBOLS, ARPA_K, ARPA_BLANK, alpha=alpha, beta=beta)
    logp, logbow = arpa_tables()
    histories = {()} | {g[:-1] for g in logp} | {g for g in logp if len(g) < 3 and g[-1] != -2}
    Q = len(model.backoff)
    assert Q == len(histories) and len(model.arc_labels) == sum(1 for g in logp if g[-1] >= 0)       # nothing of `zz` got in

    def state_of(h):
        while h not in histories:
            h = h[1:]
        return h
    nxt, wt, fin = k.sparse_lm_to_dense(model)
    # the history of every state, found by walking the expansion from the <s> history in state 0; the empty history, which no arc
    # leads to, is where state 0 backs off to
    hist_of, todo = {0: (-1,), int(model.backoff[0]): ()}, [0, int(model.backoff[0])]
    while todo:
        q = todo.pop()
        for c in range(1, ARPA_K):
            n = int(nxt[q, c])
            if n < 0:
                continue
            h1 = state_of((hist_of[q] + (c,))[-2:])
            if n not in hist_of:
                hist_of[n] = h1
                todo.append(n)
            assert hist_of[n] == h1, (q, c)
    reached = set(hist_of)
    assert len(reached) == Q and set(hist_of.values()) == histories
    # every symbol has a unigram, so no label is forbidden anywhere; the blank's column is
    worst = 0.0
    for q in sorted(reached):
        h = hist_of[q]
        assert wt[q, ARPA_BLANK] == 0 and nxt[q, ARPA_BLANK] == -1
        for c in range(1, ARPA_K):
            want = 10.0 ** (alpha * backed_off_log10(logp, logbow, h, c)) * math.exp(beta)
            worst = max(worst, abs(float(wt[q, c]) - want) / want)
        end = backed_off_log10(logp, logbow, h, -2)
        worst_f = abs(float(fin[q]) - 10.0 ** (alpha * end)) / 10.0 ** (alpha * end)
        assert worst_f <= 2.0 ** -23, (q, h)
    # a factor that backed off d <= 2 times is d + 1 float32 values and d float32 products: (2 d + 1) roundings of 2^-24 each
    assert worst <= 5.01 * 2.0 ** -24, worst
    assert (-1,) in hist_of.values() and () in hist_of.values() and (1, 2) in hist_of.values() and (3, 3) in hist_of.values()


def test_arpa_states_are_numbered_as_documented(tmp_path):
    import kaldi_lstm_amd as k
    model = k.arpa_label_lm(arpa_text(), ARPA_SYMBOLS, ARPA_K, ARPA_BLANK)
    assert model.backoff[0] == 1 and model.backoff[1] == -1               # <s> backs off to the empty history, which ends the chain
    assert np.float32(model.backoff_weight[0]) == np.float32(10.0 ** -0.40)
    off = model.arc_offsets
    assert model.arc_labels[off[0]:off[1]].tolist() == [1, 3] and off[2] - off[1] == 6        # <s> a, <s> c; all six unigrams
    assert all(np.all(np.diff(model.arc_labels[off[q]:off[q + 1]]) > 0) for q in range(len(model.backoff)))
    a_path = str(tmp_path / "lm.arpa")
    with open(a_path, "w") as fh:
        fh.write(arpa_text())
    again = k.arpa_label_lm(a_path, ["<blk>", "a", "b", "c", "d", "e", "f"], ARPA_K, ARPA_BLANK)    # a path, a list of symbols
    assert all(np.array_equal(x, y) for x, y in zip(model[1:], again[1:]))


def test_cpp_reader_writes_the_arrays_of_the_python_reader(tmp_path):
    import kaldi_lstm_amd as k
    arpa, syms, out = str(tmp_path / "lm.arpa"), str(tmp_path / "syms.txt"), str(tmp_path / "out.bin")
    with open(arpa, "w") as fh:
        fh.write(arpa_text())
    with open(syms, "w") as fh:
        fh.write("".join("%s %d\n" % kv for kv in ARPA_SYMBOLS.items()))
    for alpha, beta in ((1.0, 0.0), (0.9, 0.2)):
        model = k.arpa_label_lm(arpa, ARPA_SYMBOLS, ARPA_K, ARPA_BLANK, alpha=alpha, beta=beta)
        run_driver("arpa", arpa, syms, ARPA_K, ARPA_BLANK, alpha, beta, out)
        raw = np.fromfile(out, dtype=np.int32)
        p = 0
        for name, dtype in (("arc_offsets", np.int32), ("arc_labels", np.int32), ("arc_next", np.int32), ("arc_weight", np.float32),
                            ("backoff", np.int32), ("backoff_weight", np.float32), ("final", np.float32)):
            n = int(raw[p])
            got = raw[p + 1:p + 1 + n].view(dtype)
            p += 1 + n
            want = np.asarray(getattr(model, name), dtype)
            assert got.view(np.int32).tolist() == want.view(np.int32).tolist(), name          # the bits
        assert p == len(raw)


# ---------------------------------------------------------------------------------------------------------------------------------
# the count-based builder
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
def test_backoff_ngram_distributions_sum_to_one(order):
    """sum_c P(c | q) + P(end | q) = 1 for every state, in float64 before the cast: within 1e-9, far above K rounding errors and far
    below any modelling mistake"""
    import kaldi_lstm_amd as k
    K, blank = 9, 4
    rng = np.random.RandomState(order)
    seqs = R.markov_sequences(rng, K, blank, 50, 10)
    model = k.backoff_ngram_label_lm(seqs, K, blank, order=order, discount=0.75, alpha=1.0, beta=0.0, dtype=np.float64)
    Q = len(model.backoff)
    assert Q >= (1, 3, 10, 20, 30)[order - 1] and int(model.backoff[0]) == (1 if order > 1 else -1)
    depths = set()
    for q in range(Q):
        total = float(model.final[q])
        for c in range(K):
            g, n, d = k.sparse_lm_lookup(model, q, c, with_depth=True, dtype=np.float64)
            assert (c == blank) == (n < 0) and 0 <= float(g) <= 1
            total += float(g)
            depths.add(d)
        assert abs(total - 1.0) <= 1e-9, (q, total)
    assert depths >= set(range(order))
    cast = k.backoff_ngram_label_lm(seqs, K, blank, order=order)
    assert cast.arc_weight.dtype == np.float32 and np.array_equal(cast.arc_next, model.arc_next)
    assert k.sparse_lm_validate(cast, blank)[1][:6] == [0] * 6


def test_alpha_and_beta_are_folded_into_the_weights():
    import kaldi_lstm_amd as k
    K, blank = 6, 0
    seqs = R.markov_sequences(np.random.RandomState(7), K, blank, 30, 8)
    a = k.backoff_ngram_label_lm(seqs, K, blank, order=3, dtype=np.float64)
    b = k.backoff_ngram_label_lm(seqs, K, blank, order=3, alpha=0.7, beta=0.3, dtype=np.float64)
    assert np.allclose(b.arc_weight, a.arc_weight ** 0.7 * math.exp(0.3), rtol=1e-12)
    assert np.allclose(b.backoff_weight, a.backoff_weight ** 0.7, rtol=1e-12) and np.allclose(b.final, a.final ** 0.7, rtol=1e-12)


# ---------------------------------------------------------------------------------------------------------------------------------
# the definition of a lookup
# ---------------------------------------------------------------------------------------------------------------------------------
def test_lookup_forbids_and_multiplies_as_defined():
    import kaldi_lstm_amd as k
    F = np.float32
    m = k.SparseLm(4, np.asarray([0, 1, 2, 2]), np.asarray([1, 2]), np.asarray([2, 7]), np.asarray([0.5, 0.3], F),
                   np.asarray([1, -1, 1]), np.asarray([0.7, 1.0, 0.0], F), None)
    assert k.sparse_lm_lookup(m, 0, 1) == (F(0.5), 2)                    # an arc of the state: its weight as it is
    g, n, d = k.sparse_lm_lookup(m, 0, 2, with_depth=True)
    assert (g, n, d) == (F(F(0.7) * F(0.3)), 7, 1)                       # after a back-off: one float32 product; a bad next stays
    assert k.sparse_lm_lookup(m, 0, 3) == (F(0), -1) and k.sparse_lm_lookup(m, 1, 1) == (F(0), -1)      # a miss without a back-off
    assert k.sparse_lm_lookup(m, 2, 2) == (F(0), 7)                      # a zero back-off weight: the factor is 0
    nxt, wt, fin = k.sparse_lm_to_dense(m)
    assert nxt.tolist() == [[-1, 2, -1, -1], [-1, -1, -1, -1], [-1, -1, -1, -1]] and fin is None
    assert wt[0].tolist() == [0, 0.5, F(F(0.7) * F(0.3)), 0]
    tiny = m._replace(backoff_weight=np.asarray([2.0 ** -61, 1.0, 0.0], F))
    assert k.sparse_lm_lookup(tiny, 0, 2)[0] == 0                        # a back-off weight below 2^-60 is flushed to 0
    deep = R.chain_model(12)                                             # not validated: the walk still ends after 9 states
    assert k.sparse_lm_lookup(deep, 0, 7, with_depth=True) == (F(0), -1, 8)


def test_the_expansion_is_the_lookup_cell_by_cell():
    import kaldi_lstm_amd as k
    rng = np.random.RandomState(9)
    faint = R.counted_model(2, 12, 11, 3)
    faint = faint._replace(backoff_weight=(rng.rand(len(faint.backoff)) * 1e-9).astype(np.float32))      # products that get flushed
    for model in (R.counted_model(1, 9, 2, 5), R.explicit_model(rng, 7, 0, 6), k.sparse_lm_validate(R.chain_model(9), R.BROKEN_BLANK)[0], faint):
        nxt, wt, _ = k.sparse_lm_to_dense(model)
        Q = len(model.backoff)
        for q in range(Q):
            for c in range(model.classes):
                g, n = k.sparse_lm_lookup(model, q, c)
                assert np.float32(g).view(np.int32) == wt[q, c].view(np.int32) and nxt[q, c] == (n if 0 <= n < Q else -1), (q, c)


@pytest.mark.parametrize("name", sorted(R.broken_models()))
def test_host_mirror_of_the_build_validation(name):
    import kaldi_lstm_amd as k
    model, status = R.broken_models()[name]
    cut, got = k.sparse_lm_validate(model, R.BROKEN_BLANK)
    assert got[:6] == status and got[7] == 0
    Q = len(cut.backoff)
    assert k.sparse_lm_validate(cut, R.BROKEN_BLANK)[1][:6] == [0] * 6    # what is left is a valid model
    for q in range(Q):
        d, s = 0, int(cut.backoff[q])
        while s >= 0:
            d, s = d + 1, int(cut.backoff[s])
        assert d <= 8
    k.sparse_lm_to_dense(cut)


# ---------------------------------------------------------------------------------------------------------------------------------
# the twin
# ---------------------------------------------------------------------------------------------------------------------------------
def test_lazy_tables_and_the_expansion_give_the_same_lists():
    rng = np.random.RandomState(3)
    S, T, K, B, C, N = 3, 30, 9, 6, 4, 4
    lens = [30, 0, 17]
    y = softmax_rows(rng, T, S, K)
    refs = [[1, 2, 3], [], [4, 5]]
    for model in (R.counted_model(1, K, 2, 4), R.explicit_model(rng, K, 2, 5), R.without_final(R.counted_model(2, K, 2, 2))):
        a, _ = R.beam_twin_slm(y, lens, 2, B, C, N, model, refs=refs)
        b, tabs = R.beam_twin_slm(y, lens, 2, B, C, N, model, refs=refs, lazy=True)
        assert a == b and len(tabs.cache) > 0


@pytest.mark.parametrize("seed", R.COVERAGE_SEEDS)
def test_the_coverage_seeds_meet_the_condition(seed):
    """on the twin: lookups of every back-off depth 0 to 4 among the extensions with f > 0, and a 1-best the LM changed"""
    sh = R.COVERAGE_SHAPE
    y, lens, model = R.coverage_case(seed)
    tw, tabs = R.beam_twin_slm(y, lens, sh["blank"], sh["B"], sh["C"], sh["N"], model, lazy=True)
    missing, changed, weakest = R.coverage_findings(y, lens, model, tw, tabs)
    assert weakest >= R.STRONG            # so a lookup with a factor >= 2^-30 and a next state in range IS an extension with f > 0
    assert missing == [] and changed != [], (dict(tabs.depth), changed)


def test_a_model_of_the_training_text_lowers_the_error_count():
    """posteriors that follow label sequences of a second-order chain loosely; an order-4 model counted on other sequences of the
    same chain brings the 1-best closer to them than the search without it"""
    from tests.ctc_decode_ref import levenshtein
    K, blank, B, C = 9, 0, 8, 5
    rng = np.random.RandomState(11)
    chain = np.random.RandomState(5)
    seqs = R.markov_sequences(chain, K, blank, 260, 10, peak=0.05)
    train, test = seqs[:240], [s for s in seqs[240:] if len(s) >= 4][:10]
    import kaldi_lstm_amd as k
    model = k.backoff_ngram_label_lm(train, K, blank, order=4, alpha=1.0, beta=1.0)
    with_lm = without = 0
    for ref in test:
        frames = []
        for c in ref:
            frames += [c, c, blank]
        z = rng.randn(len(frames), 1, K) * 1.2
        for t, c in enumerate(frames):
            z[t, 0, c] += 1.6
        y = np.exp(z - z.max(-1, keepdims=True))
        y = (y / y.sum(-1, keepdims=True)).astype(np.float32)
        tw, _ = R.beam_twin_slm(y, [len(frames)], blank, B, C, 1, model, final=None, lazy=True)
        with_lm += levenshtein(tw["hyp"][0][0], ref)
        without += levenshtein(Bm.beam_twin(y, [len(frames)], blank, B, C, 1)["hyp"][0][0], ref)
    assert with_lm < without, (with_lm, without)
