"""MMI (CTC-CRF) against a label-LM denominator, host side (no GPU): the float64 yardstick of the GPU tests (tests/ctc_mmi_ref.py) is pinned
by enumeration of every frame path and by central differences of the loss, the float32 twin is held against it, the status rules are
spelled out, and the library carries the entries with their limits."""
import itertools

import numpy as np
import pytest
import torch

from tests import cpp_driver
from tests import ctc_mmi_ref as M
from tests import ctc_ref as R

# (K, blank, kind) of the grid that can be enumerated: K <= 4
SMALL_LMS = [(3, 0, "unigram"), (3, 1, "bigram"), (3, 2, "bigram"), (4, 0, "trigram"), (4, 0, "lexicon"), (4, 3, "bigram")]


def build_ctc_mmi_driver():
    return cpp_driver.build("ctc_mmi_test")


def run_driver(*args, ok=True):
    return cpp_driver.run("ctc_mmi_test", *args, ok=ok)


def _posteriors(kind, T, K, seed):
    return R.small_posteriors(kind, T, 1, K, torch.Generator().manual_seed(seed))[:, 0].numpy()


@pytest.mark.parametrize("K,blank,kind", SMALL_LMS)
def test_truth64_z_is_the_sum_over_every_path(K, blank, kind):
    lm = M.make_lm(kind, K, blank)
    worst = 0.0
    for T, post in itertools.product((1, 2, 3, 5), ("flat", "peaked")):
        y = _posteriors(post, T, K, 10 * T + K).astype(np.float64)
        z = M.enumerate_z(np.maximum(y, M.FLT_MIN), lm, blank)
        if z == 0.0:
            continue
        logz, gam = M._den_lin64(np.maximum(y, M.FLT_MIN), lm, blank)
        worst = max(worst, abs(np.exp(logz) - z) / z)
        assert np.abs(gam.sum(1) - 1).max() < 1e-12
    print(f"Z against enumeration, K {K} {kind}: {worst:.3g}", flush=True)
    assert worst <= 1e-12


def test_truth64_loss_against_enumeration_of_numerator_and_denominator():
    K, blank, T = 3, 0, 5
    lm = M.make_lm("bigram", K, blank)
    y = _posteriors("flat", T, K, 5)
    for lab in ([], [1], [1, 1], [2, 1], [1, 2, 1]):
        t = M.truth64(y[:, None], [T], [lab], lm, blank)
        yd = np.maximum(y.astype(np.float64), M.FLT_MIN)
        want = -np.log(M.enumerate_z(yd, lm, blank, lab)) - M.lm_logw(lm, blank, lab) + np.log(M.enumerate_z(yd, lm, blank))
        assert abs(t["loss"][0] - want) <= 1e-12 * max(1.0, abs(want)) and t["loss"][0] >= -1e-12, (lab, t["loss"][0], want)


@pytest.mark.parametrize("K,blank,kind,lam", [(3, 1, "bigram", 0.0), (4, 0, "trigram", 0.3), (4, 0, "lexicon", 0.0), (5, 2, "unigram", 0.5)])
def test_truth64_diff_is_the_gradient_with_respect_to_the_softmax_input(K, blank, kind, lam):
    """central differences of loss + lam * ctc loss over the softmax input, float64"""
    lm = M.make_lm(kind, K, blank)
    T = 5
    classes = [c for c in range(K) if c != blank]
    lab = [classes[0], classes[-1]] if kind != "lexicon" else [classes[0]]
    assert M.lm_logw(lm, blank, lab) > -np.inf
    a = np.random.RandomState(K).randn(T, K)

    def f(a):
        y = np.exp(a - a.max(1, keepdims=True))
        y /= y.sum(1, keepdims=True)
        o = M.objective64(y, lab, lm, blank)
        return o["loss"] + lam * (-o["num_logp"]), y, o
    _, y, o = f(a)
    diff = o["gamma_den"] - o["gamma_ref"] + lam * (y - o["gamma_ref"])
    h, worst = 1e-5, 0.0
    for t, k in itertools.product(range(T), range(K)):
        d = np.zeros_like(a)
        d[t, k] = h
        worst = max(worst, abs((f(a + d)[0] - f(a - d)[0]) / (2 * h) - diff[t, k]))
    print(f"diff against central differences, K {K} {kind} lam {lam}: {worst:.3g}", flush=True)
    assert worst <= 1e-7 and np.abs(diff).max() > 1e-3


@pytest.mark.parametrize("K,blank,kind", SMALL_LMS)
def test_plain32_stays_near_truth64(K, blank, kind):
    lm = M.make_lm(kind, K, blank)
    T = 5
    y = R.small_posteriors("flat", T, 4, K, torch.Generator().manual_seed(K)).numpy()
    classes = [c for c in range(K) if c != blank]
    labels = [[], [classes[0]], [classes[0], classes[0]], [classes[-1], classes[0]]]
    lens = [T, T, 3, 0]
    t = M.truth64(y, lens, labels, lm, blank, 0.2)
    loss, diff = M.plain32(y, lens, labels, lm, blank, 0.2)
    e, r = M.pooled_errors(loss, diff, t, lens)
    assert e < 1e-5 and r < 1e-5
    for s in range(4):
        if t["status"][s] != "counted":
            assert not diff[:, s].any() and loss[s] == (np.inf if t["status"][s] == "rejected" else 0)


def test_statuses():
    K, blank, T = 5, 0, 10
    nxt, w, fin = M.make_lm("lexicon", K, blank)            # words [1], [1, 3], [3, 3, 1]; separator 4
    lm = (nxt, w, fin)
    assert (nxt == -1).any() and (fin == 0).any()
    labels = [[1], [1], [1, 1], [2], [1, 4, 1, 3], [3, 3], [], [0, 1], [1, 5], [1]]
    lens = [10, 0, 10, 10, 4, 10, 10, 10, 10, 11]
    st = M.statuses(lens, labels, lm, K, blank, T)
    #        word    idle    "11" no word  arc next -1  fits     ends inside a word  empty: final[0] = 0  blank     outside K   len > T
    assert st == ["counted", "idle", "rejected", "rejected", "counted", "rejected", "rejected", "rejected", "rejected", "rejected"]
    assert M.statuses([2], [[1, 4, 1]], lm, K, blank, T) == ["rejected"]               # CTC feasibility: three labels in two frames
    assert M.statuses([2], [[1, 1]], M.all_ones_lm(K), K, blank, T) == ["rejected"]    # a repeat needs a blank between
    fin1 = fin.copy(); fin1[0] = 0.5
    assert M.statuses([3], [[]], (nxt, w, fin1), K, blank, T) == ["counted"]           # the empty reference with final[0] > 0
    w0 = w.copy(); w0[0, 1] = 0
    assert M.statuses([3], [[1]], (nxt, w0, fin), K, blank, T) == ["rejected"]         # a weight of 0
    w0[0, 1] = np.nan
    assert M.statuses([3], [[1]], (nxt, w0, fin), K, blank, T) == ["rejected"]         # ... or NaN
    assert M.statuses([3], [[1]], (nxt, w, None), K, blank, T) == ["counted"]          # final None: all ones
    assert M.statuses([2], [[3, 3]], (nxt, w, None), K, blank, T) == ["rejected"]      # two equal labels need a blank between them
    assert M.statuses([3], [[3, 3]], (nxt, w, None), K, blank, T) == ["counted"]       # ... with it, and final None, a prefix of a word
    t = M.truth64(np.full((T, 1, K), 0.2, np.float32), [10], [[2]], lm, blank)
    assert t["loss"][0] == np.inf and not t["diff"].any()


def test_all_ones_lm_is_ctc():
    """Q = 1, all weights 1: Z = prod_t (row sum) = 1, gamma_den = y, loss = the CTC loss, diff = (1 + lam) (y - gamma_ref)"""
    K, blank, T = 4, 0, 6
    y32 = R.small_posteriors("flat", T, 2, K, torch.Generator().manual_seed(2)).numpy()
    labels, lens = [[1, 2], [3, 3]], [T, 5]
    for s in range(2):
        y = y32[:lens[s], s].astype(np.float64)
        y /= y.sum(1, keepdims=True)                                             # rows that sum to 1 in float64
        o = M.objective64(y, labels[s], M.all_ones_lm(K), blank)
        assert abs(o["logz"]) < 1e-12 and o["logw"] == 0 and abs(o["loss"] + o["num_logp"]) < 1e-12
        assert np.abs(o["gamma_den"] - y).max() < 1e-12
    # on float32 rows Z is the product of the row sums, which the CTC loss of the raw posteriors does not see
    t = M.truth64(y32, lens, labels, M.all_ones_lm(K), blank, 0.5)
    l64, d64 = R.truth64(y32, lens, labels, blank)
    for s in range(2):
        rows = np.log(y32[:lens[s], s].astype(np.float64).sum(1)).sum()
        assert abs(t["logz"][s] - rows) < 1e-12 and abs(t["loss"][s] - l64[s] - rows) < 1e-12
    assert np.abs(t["diff"] - 1.5 * d64).max() < 1e-6


def test_abi_exports_and_limits():
    import kaldi_lstm_amd as k
    lib = k.load_library()
    for name in ("klstm_ctc_mmi_graph_bytes", "klstm_ctc_mmi_graph_build", "klstm_ctc_mmi_workspace_bytes", "klstm_ctc_mmi_eval"):
        assert hasattr(lib, name), name
    g, q = lib.klstm_ctc_mmi_graph_bytes, lib.klstm_ctc_mmi_workspace_bytes
    for a in [(1, 2), (128, 128), (1, 16384), (8192, 2), (128, 127), (601, 24)]:
        assert g(*a) > 0, a
    for a in [(129, 128), (1, 16385), (0, 4), (4, 1), (-1, 4), (16385, 1)]:
        assert g(*a) == 0 and b"klstm_ctc_mmi_graph_bytes" in lib.klstm_last_error(), a
    for a in [(2047, 32, 128, 128, 1023), (65535, 1, 2, 1, 0), (1, 1, 48, 49, 10)]:
        assert q(*a) > 0, a
    for a in [(2048, 32, 4, 4, 10), (10, 33, 4, 4, 10), (10, 4, 4, 4, 1024), (0, 4, 4, 4, 10), (10, 4, 4, 4, -1), (10, 4, 128, 129, 10),
              (10, 4, 1, 4, 10), (10, 4, 4, 0, 10)]:
        assert q(*a) == 0 and b"klstm_ctc_mmi_workspace_bytes" in lib.klstm_last_error(), a
    # the reference's rows as klstm_ctc_eval keeps them and 2 * T*S * Q*K floats for the denominator's, with a bounded head
    T, S, K, Q, L = 1000, 16, 48, 49, 150
    rows = 2 * T * S * (Q * K + 304) * 4
    assert rows <= q(T, S, K, Q, L) <= rows + (1 << 20)
    assert q(T, S, K, Q, L) > q(T, S, K, Q, L - 2) and q(T, S, K, Q, L) > q(T, S, K, Q - 1, L)
    with pytest.raises(k.KlstmError) as ei:
        k.ctc_mmi_workspace_bytes(10, 4, 128, 129, 10)
    assert ei.value.status == 2


def test_cpp_driver_builds():
    r = run_driver(ok=False)
    assert r.returncode == 2 and "usage: ctc_mmi_test" in r.stderr
