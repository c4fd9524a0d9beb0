"""tests/output_tail_ref.py pinned (no GPU): truth64 against torch in float64 and against oracle/components.py, the twin against the
truth, and the conditions that keep tests/test_output_tail_gpu.py from hiding a failure behind its exclusion rule."""
import numpy as np
import pytest
import torch

from oracle import components as oc
from tests import output_tail_ref as R

WIDTHS = (3, 4, 11, 255, 256, 257, 2044, 2048, 2052, 4092, 4096, 4098, 4100, 16624, 32764, 32768, 32772)


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("cols", (3, 37, 257, 2052))
def test_truth64_is_torch_float64(regime, cols):
    a = R.logits(regime, 5, cols)
    ta = torch.from_numpy(a).double()
    ls = torch.log_softmax(ta, 1).numpy()
    assert np.abs(R.log_softmax64(a) - ls).max() <= 1e-12 * max(1.0, np.abs(ls).max())
    sm = torch.softmax(ta, 1).numpy()
    assert np.abs(R.softmax64(a) - sm).max() <= 1e-14
    lp = np.log(np.random.RandomState(cols).dirichlet(np.ones(cols))).astype(np.float32)
    assert np.array_equal(R.score64(a, R.POSTERIOR), R.softmax64(a)) and np.array_equal(R.score64(a, R.LOGPOST), R.log_softmax64(a))
    assert np.abs(R.score64(a, R.LOGLIKE, lp, 0.7) - (ls - float(np.float32(0.7)) * lp.astype(np.float64))).max() <= 1e-11


@pytest.mark.parametrize("cols", (11, 37, 129))
def test_truth64_is_the_oracle_on_small_shapes(cols):
    """softmax and Xent::EvalMasked, one-hot and general posteriors, against oracle/components.py run in float64"""
    rng = np.random.RandomState(cols)
    rows = 6
    a = R.logits("trained", rows, cols)
    assert np.abs(R.softmax64(a) - oc.softmax(a.astype(np.float64))).max() <= 1e-15
    y = R.softmax32(a)
    target = rng.randint(0, cols, rows).astype(np.int32)
    mask = np.array([1, 0, 1, 0.5, 1, 1], np.float32)
    diff, rx, correct, valid = R.xent64(y, target, mask)
    d_o, xe_o, _, c_o, v_o = oc.xent_eval_masked(y.astype(np.float64), target, mask.astype(np.float64))
    assert np.array_equal(diff, d_o) and abs(rx.sum() - xe_o) <= 1e-12 * abs(xe_o) and (int(correct.sum()), valid) == (c_o, v_o)
    assert np.array_equal(R.diff32(y, target, mask), oc.xent_eval_masked(y, target, mask)[0])
    assert np.abs(R.xent_from_logits64(a, target, mask) - (-mask * np.log(R.softmax64(a)[np.arange(rows), target]))).max() <= 1e-12
    post = [[(int(p), float(np.float32(w))) for p, w in zip(rng.randint(0, cols, n), rng.rand(n))] for n in (0, 1, 3, 7, 2, 20)]
    xe, en, correct = R.xent_post64(y, post, mask)
    d_o, xe_o, en_o, c_o, _ = oc.xent_eval_masked_post(y.astype(np.float64), post, mask.astype(np.float64))
    assert abs(xe.sum() - xe_o) <= 1e-12 * abs(xe_o) and abs(en.sum() - en_o) <= 1e-12 * abs(en_o)
    assert int(correct.sum()) == oc.xent_eval_masked_post(y, post, mask)[3]
    d32, xe32, en32 = R.xent_post32(y, post, mask)
    assert np.array_equal(d32, oc.xent_eval_masked_post(y, post, mask)[0])
    assert R.scalar_rel(xe32, xe) <= 2.0 ** -20 and R.scalar_rel(en32, en) <= 2.0 ** -20
    # out-of-range targets subtract nothing and cost nothing
    bad = np.array([-1, cols, 0, -1, cols, 1], np.int32)
    diff, rx, correct, _ = R.xent64(y, bad, mask)
    assert np.array_equal(diff[[0, 1, 3, 4]], (y.astype(np.float64) * mask[:, None].astype(np.float64))[[0, 1, 3, 4]])
    assert not rx[[0, 1, 3, 4]].any() and not correct[[0, 1, 3, 4]].any()


@pytest.mark.parametrize("cols", WIDTHS)
def test_exclusion_rule_hides_nothing(cols):
    """The relative measure leaves out true values below 2^-102.  flat and trained rows lose nothing to that; a wide row loses at most
    0.35 of its elements (the twin: <= 0.28 at 11 ... 32768 columns), never its arg-max, and the GPU tests draw targets of wide rows
    from the counted columns (output_tail_ref.targets_for); what the twin returns for an excluded element is <= 2^-101; and the twin itself is within
    2^-18 + 2^-21 of the truth on the counted elements (a - max is rounded to float32 at a size below 128: half an ulp is 2^-18 in the
    argument of exp, hence relative in its value; eight more roundings of 2^-24 for exp, the sum, 1 / sum and the product) and within
    2^-21 on the log forms, whose measure is relative to max(1, |value|)."""
    rows = 8
    for regime in ("flat", "trained", "wide"):
        a = R.logits(regime, rows, cols)
        t = R.softmax64(a)
        out = ~R.counted(t)
        share = out.mean(1).max()
        assert share == 0.0 if regime != "wide" else share <= 0.35, (regime, share)
        if cols >= 11 and regime == "wide":
            assert share <= 0.28
        assert not out[np.arange(rows), t.argmax(1)].any()
        tw = R.softmax32(a)
        assert (tw[out] <= R.TINY_OUT).all()
        assert R.rel_err(tw, t) <= 2.0 ** -18 + 2.0 ** -21
        assert R.log_err(R.score32(a, R.LOGPOST), R.log_softmax64(a)) <= 2.0 ** -21
        tgt = R.targets_for(a)
        assert not out[np.arange(rows), tgt].any()
    a = R.logits("saturated", rows, cols)
    y = R.softmax32(a)
    assert set(np.unique(y)) == {0.0, 1.0} and (y.sum(1) == 1).all()          # judged by exact conditions only
    assert np.array_equal(R.score32(a, R.LOGPOST), a - a.max(1, keepdims=True))


def test_measures():
    t = np.array([[0.5, 2.0 ** -103, 0.25]])
    assert R.rel_err(np.array([[0.5, 1.0, 0.25]], np.float32), t) == 0.0                     # the excluded element is not seen ...
    assert R.rel_err(np.array([[0.5, 0.0, 0.2500001]], np.float32), t) > 1e-7               # ... a small counted one is
    assert R.scalar_rel([np.inf, np.nan, 0.0], [np.inf, np.nan, 0.0]) == 0.0
    assert R.scalar_rel([1.0], [np.inf]) == np.inf and R.scalar_rel([np.nan], [1.0]) == np.inf
    A = np.array([[1.0, -1.0]]); B = np.array([[1.0], [1.0]])
    assert R.product_err(np.array([[2.0 ** -24]], np.float32), A, B) == 2.0 ** -25           # |A||B| = 2 although A B = 0
    assert R.ulp32(1.0) == 2.0 ** -23
