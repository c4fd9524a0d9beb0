"""The output layer's kernels on the device against float64 (tests/output_tail_ref.py) at every edge of their dispatch: AffineTransform
(klstm_affine_*), Softmax, Xent::EvalMasked in its three forms, the one-pass softmax + loss kernel and the scorer's log-softmax scatter.
THE BARS.  Posteriors: max |gpu - truth64| / truth64 over the true values >= 2^-102 (tests/test_output_tail.py shows what that leaves out);
log forms: |gpu - truth64| / max(1, |truth64|); both at most max(4 x the same error of twin32, 2^-21) -- 4 is the suite's margin for another
expf and summation tree (test_ctc_small_gpu.py), 2^-21 eight float32 roundings of a value <= 1.  row_xent, in ulps of the truth:
max(4 x twin, 2).  Every such pair of errors is the largest over the calls of one (entry, regime, width class).  Derivatives of a given posterior, the statistics, and everything the one-pass kernel shares with the pair: exact.
Products: componentwise, max_ij |C - C64|_ij / (|A| |B|)_ij <= max(4 x numpy's float32 product, floor), floor 2^-21 where the f16 x 2
kernel runs (two fp16 planes per operand: 22 significant bits a side; the dispatch predicates are restated here and held against
the bits) and 2^-22 on every fp32 kernel.
Measured figures: profiles/output_tail_parity_margins.json."""
import functools
import math

import numpy as np
import pytest
import torch

import kaldi_lstm_amd as k
from kaldi_lstm_amd.binding import load_library
from oracle import components as oc
from tests import output_tail_ref as R
from tests.margins import bound

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -21
SENT = 7.0
WIDTHS = (3, 4, 255, 256, 257, 2044, 2048, 2052, 4092, 4096, 4098, 4100, 16624, 32764, 32768, 32772)
# layout = (column offset of the view, row stride - cols): contiguous; a column window; an odd row stride; a base one float in
CONTIG, WINDOW, ODD, OFF1 = (0, 0), (0, 4), (0, 1), (1, 4)
# (input, output / diff, post): each line after the first two flips ONE conjunct of the wide kernels' predicate for ONE matrix
LAYOUTS = {"contiguous": (CONTIG, CONTIG, CONTIG), "window": (WINDOW, WINDOW, WINDOW),
           "in_odd_stride": (ODD, WINDOW, WINDOW), "out_odd_stride": (WINDOW, ODD, WINDOW), "post_odd_stride": (WINDOW, WINDOW, ODD),
           "in_off_one": (OFF1, WINDOW, WINDOW), "out_off_one": (WINDOW, OFF1, WINDOW), "post_off_one": (WINDOW, WINDOW, OFF1)}


def wide_shape(cols):
    return cols % 4 == 0 and 2048 <= cols <= 32768


def aligned(layout):
    return layout[0] % 4 == 0 and layout[1] % 4 == 0


class Buf:
    """a [rows, cols] view into a [rows + 1, cols + pad] matrix of sentinels (one sentinel row, sentinel columns where the layout has any)"""

    def __init__(self, rows, cols, layout, data=None):
        off, pad = layout
        self.whole = torch.full((rows + 1, cols + pad), SENT, device="cuda")
        self.v = self.whole[:rows, off:off + cols]
        assert self.v.data_ptr() % 16 == (4 * off) % 16 and self.v.stride(0) == cols + pad
        if data is not None:
            self.v.copy_(torch.from_numpy(np.ascontiguousarray(data)))
        self.before = self.whole.clone() if data is not None else None

    def get(self, written=None):
        """the view as numpy, after checking that nothing outside it (an input: nothing at all) changed; written: bool per row"""
        torch.cuda.synchronize()
        out = self.v.cpu().numpy().copy()
        if self.before is not None:
            assert torch.equal(self.whole, self.before), "an input matrix was written"
            return out
        chk = self.whole.clone()
        off = (self.v.data_ptr() - self.whole.data_ptr()) // 4
        chk[:self.v.shape[0], off:off + self.v.shape[1]] = SENT
        assert bool((chk == SENT).all()), "memory outside the view was written"
        if written is not None:
            assert bool((self.v[~torch.from_numpy(written).cuda()] == SENT).all()), "a row that is not a destination was written"
        return out


def i32(a):
    return torch.from_numpy(np.asarray(a, np.int32)).cuda()


def f32(a):
    return torch.from_numpy(np.asarray(a, np.float32)).cuda()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def masks(rows):
    return np.array([1.0, 1.0, 0.0, 0.5, 1.0, 1.0, 0.5, 0.0] * (rows // 8 + 1), np.float32)[:rows]


def log_prior(cols):
    return np.log(np.random.RandomState(cols).dirichlet(np.full(cols, 2.0)) + 1e-12).astype(np.float32)


def gpu_rows(a, target, mask, lay=LAYOUTS["contiguous"]):
    """every row entry once on logits a: the pair (softmax, then xent_eval_masked on the device's own posterior), the one-pass kernel with
    and without the posterior output and with and without device totals (all four), and the three scorer modes.  Returns numpy outputs; sentinels are checked on the way."""
    rows, cols = a.shape
    lin, lout, lpost = lay
    tg, mk = i32(target), f32(mask)
    o = {}
    ain = Buf(rows, cols, lin, a)
    y = Buf(rows, cols, lpost)                               # the pair through the same three layouts as the one-pass entry: the same kernels
    k.softmax(ain.v, y.v)
    o["y"] = y.get()
    ain.get()
    d = Buf(rows, cols, lout)
    rx, rc = torch.full((rows + 1,), SENT, device="cuda"), torch.full((rows + 1,), SENT, device="cuda")
    o["stats"] = k.xent_eval_masked(y.v, tg, mk, d.v, rows_out=(rx[:rows], rc[:rows]))
    o["diff"], o["rx"], o["rc"] = d.get(), rx[:rows].cpu().numpy(), rc[:rows].cpu().numpy()
    assert same_bits(y.get(), o["y"]), "Xent::EvalMasked wrote its input"
    assert rx[rows].item() == SENT and rc[rows].item() == SENT
    # one pass, posterior written
    d1, p1 = Buf(rows, cols, lout), Buf(rows, cols, lpost)
    rx1, rc1 = torch.full((rows + 1,), SENT, device="cuda"), torch.full((rows + 1,), SENT, device="cuda")
    o["stats1"] = k.softmax_xent_masked(ain.v, tg, mk, d1.v, post=p1.v, rows_out=(rx1[:rows], rc1[:rows]))
    o["diff1"], o["post1"], o["rx1"], o["rc1"] = d1.get(), p1.get(), rx1[:rows].cpu().numpy(), rc1[:rows].cpu().numpy()
    assert rx1[rows].item() == SENT and rc1[rows].item() == SENT
    # one pass, posterior written AND statistics onto device totals (the kernel's own last-workgroup sum where it runs, klstm_xent_accumulate
    # behind the two-kernel fall-back elsewhere), twice onto the same totals
    d3, p3 = Buf(rows, cols, lout), Buf(rows, cols, lpost)
    rx3, rc3 = torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
    tot = torch.zeros(3, dtype=torch.float64, device="cuda")
    o["tot3"] = []
    for _ in range(2):
        assert k.softmax_xent_masked(ain.v, tg, mk, d3.v, post=p3.v, rows_out=(rx3, rc3), totals=tot) == (None, None, None)
        torch.cuda.synchronize()
        o["tot3"].append(tot.cpu().numpy())
    o["diff3"], o["post3"], o["rx3"], o["rc3"] = d3.get(), p3.get(), rx3.cpu().numpy(), rc3.cpu().numpy()
    # one pass, no posterior, with and without totals: only where the one-pass kernel itself runs; elsewhere the entry says that it needs
    # the buffer
    d2, d4 = Buf(rows, cols, lout), Buf(rows, cols, lout)
    rx2, rc2 = torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
    rx4, rc4 = torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
    tot = torch.zeros(3, dtype=torch.float64, device="cuda")
    if wide_shape(cols) and aligned(lin) and aligned(lout):
        k.softmax_xent_masked(ain.v, tg, mk, d2.v, rows_out=(rx2, rc2), totals=tot)
        stats4 = k.softmax_xent_masked(ain.v, tg, mk, d4.v, rows_out=(rx4, rc4))
        if aligned(lpost):                                   # (else the pair above went through the narrow kernels: other bits)
            o["stats4"] = stats4
            o["diff2"], o["rx2"], o["rc2"], o["tot2"] = d2.get(), rx2.cpu().numpy(), rc2.cpu().numpy(), tot.cpu().numpy()
            o["diff4"], o["rx4"], o["rc4"] = d4.get(), rx4.cpu().numpy(), rc4.cpu().numpy()
    else:
        with pytest.raises(k.KlstmError):
            k.softmax_xent_masked(ain.v, tg, mk, d2.v, rows_out=(rx2, rc2))
        d2.get()
    ain.get()
    # the scorer: rows scattered in reverse into a matrix with two more rows, row 0 dropped (-1)
    dst = np.arange(rows + 1, 1, -1, dtype=np.int32)
    dst[0] = -1
    written = np.zeros(rows + 2, bool)
    written[dst[1:]] = True
    lp = f32(log_prior(cols))
    for mode in (R.POSTERIOR, R.LOGPOST, R.LOGLIKE):
        sc = Buf(rows + 2, cols, lout)
        k.log_softmax_scatter(ain.v, i32(dst), sc.v, mode, log_prior=lp if mode == R.LOGLIKE else None, prior_scale=0.7)
        o["score", mode] = sc.get(written)[dst[1:]]            # rows 1 .. of the input, in input order
    ain.get()
    o["same_class"] = aligned(lout) == aligned(lpost)        # the scorer's output and Softmax's went through the same kind of kernel
    return o


def exact_parts(o, a, target, mask):
    """what needs no tolerance: the derivative of a given posterior, the statistics, one pass == the pair"""
    rows, cols = a.shape
    y = o["y"]
    assert same_bits(o["diff"], R.diff32(y, target, mask)), "diff != (y - onehot) * mask in float32"
    _, _, correct, valid = R.xent64(y, target, mask)
    assert np.array_equal(o["rc"], correct)
    assert o["stats"][1:] == (int(correct.sum()), valid)
    for s in ("1", "2", "3", "4"):                           # post; totals; post and totals; neither
        if "diff" + s in o:
            assert same_bits(o["diff" + s], o["diff"]), f"one pass ({s}): diff differs from the pair's"
            assert np.array_equal(o["rx" + s], o["rx"], equal_nan=True) and np.array_equal(o["rc" + s], o["rc"]), f"one pass ({s}): rows differ"
    assert same_bits(o["post1"], y) and same_bits(o["post3"], y)
    for s in ("stats1", "stats4"):
        if s in o:
            assert o[s][1:] == o["stats"][1:]
            assert o[s][0] == o["stats"][0] or (math.isnan(o[s][0]) and math.isnan(o["stats"][0]))
    # device totals against the double sum of the returned rows (worst case of a sum of n doubles: n 2^-53 sum |x|)
    x = o["rx"].astype(np.float64)
    checks = [(f"with post, launch {n}", o["tot3"][n - 1], n) for n in (1, 2)]
    if "tot2" in o:
        checks.append(("without post", o["tot2"], 1))
    for name, tot, n in checks:
        assert tot[1] == n * correct.sum() and tot[2] == n * float(mask.astype(np.float64).sum()), name
        if np.isfinite(x).all():
            bound(abs(tot[0] - n * math.fsum(x)), n * rows * 2.0 ** -53 * np.abs(x).sum() + 5e-324, f"totals[0] {name}")
        else:
            assert not np.isfinite(tot[0]), name
    if o["same_class"]:
        assert same_bits(o["score", R.POSTERIOR], y[1:]), "the scorer's posterior is not Softmax's"
    # out-of-range targets: nothing subtracted, no loss, never correct
    bad = (target < 0) | (target >= cols)
    assert same_bits(o["diff"][bad], (y * mask[:, None])[bad]) and not o["rx"][bad].any() and not o["rc"][bad].any()
    assert not o["diff"][mask == 0].any() and not o["rc"][mask != 1].any()


def accuracy_parts(o, a, target, mask):
    """the measures of the module docstring for one call: [(what, the device's error, the twin's, floor)]"""
    rows, cols = a.shape
    lp = log_prior(cols)
    figs = []
    t = R.softmax64(a)
    tw = R.softmax32(a)
    for name, what in (("y", "softmax"), ("post1", "one-pass posterior")):
        figs.append((what, R.rel_err(o[name], t), R.rel_err(tw, t), FLOOR))
        assert (o[name][~R.counted(t)] <= R.TINY_OUT).all(), (cols, name, "an excluded element is not small")
    # (the scorer drops row 0: its twin is judged on the same rows)
    figs.append(("scorer posterior", R.rel_err(o["score", R.POSTERIOR], t[1:]), R.rel_err(tw[1:], t[1:]), FLOOR))
    assert (o["score", R.POSTERIOR][~R.counted(t[1:])] <= R.TINY_OUT).all()
    for mode, what in ((R.LOGPOST, "scorer log-posterior"), (R.LOGLIKE, "scorer log-likelihood")):
        t64 = R.score64(a, mode, lp, 0.7)
        figs.append((what, R.log_err(o["score", mode], t64[1:]), R.log_err(R.score32(a, mode, lp, 0.7)[1:], t64[1:]), FLOOR))
    # row_xent in ulps of the truth: the pair's from the device's float32 posterior, the one-pass kernel's from the logits
    y = o["y"]
    rx64 = R.xent64(y, target, mask)[1]
    figs.append(("row_xent (ulps of the truth)", float((np.abs(o["rx"] - rx64) / R.ulp32(rx64)).max()),
                 float((np.abs(R.xent32(y, target, mask) - rx64) / R.ulp32(rx64)).max()), 2.0))
    rx64 = R.xent_from_logits64(a, target, mask)
    figs.append(("one-pass row_xent (ulps of the truth)", float((np.abs(o["rx1"] - rx64) / R.ulp32(rx64)).max()),
                 float((np.abs(R.xent32(tw, target, mask) - rx64) / R.ulp32(rx64)).max()), 2.0))
    return figs


def settle(figs, tag):
    """bar = max(4 x the twin's error, floor), both errors the largest over the calls of one (entry, regime, width class); every figure is
    printed before the first is asserted"""
    pooled = {}
    for what, err, twin, floor in figs:
        e, t, _ = pooled.get(what, (0.0, 0.0, floor))
        pooled[what] = (max(e, err) if err == err else err, max(t, twin), floor)
    for what, (e, t, floor) in pooled.items():
        print(f"{tag} {what}: {e:.3g} (twin {t:.3g}, bar {max(4 * t, floor):.3g})", flush=True)
    for what, (e, t, floor) in pooled.items():
        bound(e, max(4 * t, floor), f"{tag} {what}")


FLIPPED = [n for n in LAYOUTS if n not in ("contiguous", "window")]
CLASSES = {"narrow": [(c, "contiguous") for c in WIDTHS if not wide_shape(c)],
           "wide": [(c, "contiguous") for c in WIDTHS if wide_shape(c)] + [(4096, "window"), (16624, "window")],
           "wide shape on the narrow kernel": [(c, n) for c in (4096, 16624) for n in FLIPPED]}


@pytest.mark.parametrize("regime", ("flat", "trained", "wide"))
@pytest.mark.parametrize("cols", WIDTHS)
def test_row_kernels_at_every_width(regime, cols):
    """both sides of every edge of `cols % 4 == 0 && 2048 <= cols <= 32768`, n4 = 1023 / 1024 / 1025 (last thread idle, one float4 each, one
    thread two), the widest row, and 4098 (wide but not a multiple of 4), in three logit regimes: everything that is exact"""
    a = R.logits(regime, 8, cols)
    target, mask = R.targets_for(a), masks(8)
    exact_parts(gpu_rows(a, target, mask), a, target, mask)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("cols", (4096, 16624))
def test_row_kernels_in_every_layout(cols, layout):
    """each conjunct of the wide predicate flipped on its own -- an odd row stride under wide aligned columns, a base one float in -- for
    the input, the output / diff and the posterior matrix separately.  A misaligned `post` alone sends the one-pass entry through its
    two-kernel fall-back, which must still give the pair's bits.  Everything that is exact."""
    a = R.logits("trained", 8, cols, seed=1)
    target, mask = R.targets_for(a), masks(8)
    exact_parts(gpu_rows(a, target, mask, LAYOUTS[layout]), a, target, mask)


@pytest.mark.parametrize("regime", ("flat", "trained", "wide"))
@pytest.mark.parametrize("klass", list(CLASSES))
def test_row_kernel_accuracy(klass, regime):
    """the bars, per (entry, regime, width class): the device's largest error over the widths (or layouts) of the class against 4 x the
    twin's largest over the same calls.  Every call has logits of its own (seed = its place in the class): -log(p) of a posterior next to 1
    turns the one rounding of p into hundreds of ulps of the result, so a twin judged on few rows may be lucky; over the 32 or more hot
    rows of a class its largest error is the recipe's."""
    figs = []
    for seed, (cols, layout) in enumerate(CLASSES[klass]):
        a = R.logits(regime, 8, cols, seed=seed)
        target, mask = R.targets_for(a), masks(8)
        figs += accuracy_parts(gpu_rows(a, target, mask, LAYOUTS[layout]), a, target, mask)
    settle(figs, f"{regime} / {klass}:")


def plant(regime, cols, targets, hot):
    """rows of `regime` with the given targets; where hot[r], the row's largest logit is moved onto the target column"""
    a = R.logits(regime, len(targets), cols, seed=2)
    for r, (t, h) in enumerate(zip(targets, hot)):
        if h and 0 <= t < cols:
            m = a[r].argmax()
            a[r, [t, m]] = a[r, [m, t]]
    return a


@pytest.mark.parametrize("regime", ("flat", "trained", "saturated"))
@pytest.mark.parametrize("cols,layout", [(257, "contiguous"), (4100, "contiguous"), (16624, "contiguous"), (16624, "in_odd_stride")])
def test_planted_targets_and_masks(regime, cols, layout):
    """the target on thread, slot and wave boundaries of the wide kernels (columns 0, 3, 4, 4095, 4096, 4099, cols - 4, cols - 1) and out of
    range (-1, cols), each with mask 1, 0.5 and 0, hot (the row's maximum) and cold.  saturated rows: posteriors exactly 0.0 / 1.0, row_xent
    exactly 0 on a hot target, +inf on a cold one, and NaN on a cold target of a masked row: the reference's 0 x -inf (nnet-loss.cc:122-128
    multiplies log(y) = -inf by the mask 0), which oracle.components.xent_eval_masked returns too."""
    cand = [c for c in (0, 3, 4, 4095, 4096, 4099, cols - 4, cols - 1) if c < cols] + [-1, cols]
    cases = [(t, m, h) for t in cand for m in (1.0, 0.5, 0.0) for h in (True, False)]
    figs = []
    for b in range(0, len(cases), 8):
        part = cases[b:b + 8]
        target = np.array([c[0] for c in part], np.int32)
        mask = np.array([c[1] for c in part], np.float32)
        hot = np.array([c[2] for c in part])
        a = plant(regime, cols, target, hot)
        o = gpu_rows(a, target, mask, LAYOUTS[layout])
        exact_parts(o, a, target, mask)
        inr = (target >= 0) & (target < cols)
        if regime != "flat":                                 # (a flat row has no column that stands out)
            assert np.array_equal(o["rc"], ((mask == 1) & hot & inr).astype(np.float32))
        if regime != "saturated":
            figs += accuracy_parts(o, a, target, mask)
            continue
        y = o["y"]
        assert set(np.unique(y)) <= {0.0, 1.0} and (y.sum(1) == 1).all() and (y[np.arange(len(part)), a.argmax(1)] == 1).all()
        assert same_bits(o["score", R.LOGPOST], (a - a.max(1, keepdims=True))[1:])        # log(sum) = log(1) = 0
        rx = o["rx"]
        assert np.array_equal(rx, R.xent32(y, target, mask), equal_nan=True)
        assert (rx[inr & hot] == 0).all() and (rx[inr & ~hot & (mask > 0)] == np.inf).all() and np.isnan(rx[inr & ~hot & (mask == 0)]).all()
        for r in np.flatnonzero(inr & ~hot & (mask == 0)):
            assert np.isnan(oc.xent_eval_masked(y[r:r + 1], target[r:r + 1], mask[r:r + 1])[1])
    settle(figs, f"{regime} / {cols} columns, {layout}, planted:")


@pytest.mark.parametrize("regime", ("flat", "trained", "saturated"))
@pytest.mark.parametrize("cols,layout", [(257, "contiguous"), (16624, "contiguous"), (16624, "out_off_one")])
def test_arg_max_ties_take_the_lowest_index(cols, layout, regime):
    """two equal maxima with the target on the lower and on the higher column: same thread and float4; neighbouring lanes; one thread's two
    slots (c and c + 4096); a lower column held by a higher thread of the same wave (4100 in thread 1, 8 in thread 2) and of another wave
    (4100 in thread 1, 256 in thread 64); and a constant row.  flat rows carry 5.0 on both columns, trained and saturated rows their own
    largest logit (+12, +200: both posteriors of a saturated row are exactly 0.5).  The lowest index wins in all three kernels."""
    pairs = [(8, 9), (8, 12), (40, 4136), (8, 4100), (256, 4100)] if cols > 4136 else [(8, 9), (8, 12), (40, 200), (3, 256), (63, 64)]
    cases = [(lo, hi, t) for lo, hi in pairs for t in (lo, hi)] + [(None, None, 0), (None, None, cols - 1)]
    for b in range(0, len(cases), 8):
        part = cases[b:b + 8]
        a = R.logits(regime, len(part), cols, seed=3)
        for r, (lo, hi, _) in enumerate(part):
            if lo is None:
                a[r] = np.float32(0.25)
                continue
            h = a[r].argmax()
            top = np.float32(5.0) if regime == "flat" else a[r, h]
            a[r, h] = 0
            a[r, [lo, hi]] = top
        target = np.array([c[2] for c in part], np.int32)
        mask = np.ones(len(part), np.float32)
        o = gpu_rows(a, target, mask, LAYOUTS[layout])
        exact_parts(o, a, target, mask)
        y = o["y"]
        for r, (lo, hi, t) in enumerate(part):
            if lo is None:
                assert (y[r] == y[r, 0]).all()
                continue
            assert y[r, lo] == y[r, hi] == y[r].max() and (np.delete(y[r], [lo, hi]) < y[r, lo]).all(), "the tie did not survive the softmax"
            if regime == "saturated":
                assert y[r, lo] == 0.5 and not np.delete(y[r], [lo, hi]).any()
        want = np.array([1.0 if t == (lo or 0) else 0.0 for lo, hi, t in part], np.float32)
        for s in ("rc", "rc1", "rc3"):
            assert np.array_equal(o[s], want), (s, o[s], want)


@pytest.mark.parametrize("rows", (1, 1023, 1024, 1025, 2049))
def test_one_pass_totals(rows):
    """the statistics that the last workgroup of the one-pass launch adds to `totals`: its loop over the rows (1024 threads) runs once,
    exactly once and more than once; two launches onto the same totals show that the ticket is back at zero after the first"""
    cols = 2048
    a = R.logits("trained", rows, cols, seed=4)
    target = np.random.RandomState(rows).randint(-1, cols + 1, rows).astype(np.int32)
    mask = masks(rows)
    ad, diff = f32(a), torch.empty(rows, cols, device="cuda")
    rx, rc = torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
    tot = torch.zeros(3, dtype=torch.float64, device="cuda")
    for launch in (1, 2):
        k.softmax_xent_masked(ad, i32(target), f32(mask), diff, rows_out=(rx, rc), totals=tot)
        torch.cuda.synchronize()
        x = rx.cpu().numpy().astype(np.float64)
        got = tot.cpu().numpy()
        assert got[1] == launch * rc.cpu().numpy().astype(np.float64).sum() and got[2] == launch * mask.astype(np.float64).sum()
        bound(abs(got[0] - launch * math.fsum(x)), launch * rows * 2.0 ** -53 * np.abs(x).sum(), f"totals[0] after launch {launch}")
    y = torch.empty(rows, cols, device="cuda")
    k.softmax(ad, y)
    torch.cuda.synchronize()
    assert np.array_equal(rc.cpu().numpy(), R.xent64(y.cpu().numpy(), target, mask)[2])


# ---- general posteriors ----
def gpu_post(y, post, mask, lay=(CONTIG, WINDOW)):
    rows, cols = y.shape
    off = np.cumsum([0] + [len(fr) for fr in post]).astype(np.int32)
    pdf = np.array([p for fr in post for p, _ in fr] or [0], np.int32)
    w = np.array([w_ for fr in post for _, w_ in fr] or [0.0], np.float32)
    yin, d = Buf(rows, cols, lay[0], y), Buf(rows, cols, lay[1])
    outs = [torch.full((rows + 1,), SENT, device="cuda") for _ in range(3)]
    offd, pdfd, wd, mk = i32(off), i32(pdf), f32(w), f32(mask)
    st = load_library().klstm_xent_eval_masked_post(yin.v.data_ptr(), rows, cols, yin.v.stride(0), offd.data_ptr(), pdfd.data_ptr(), wd.data_ptr(),
                                                    mk.data_ptr(), d.v.data_ptr(), d.v.stride(0), outs[0].data_ptr(), outs[1].data_ptr(),
                                                    outs[2].data_ptr(), None)
    assert st == 0, load_library().klstm_last_error()
    diff = d.get()
    yin.get()
    assert all(t[rows].item() == SENT for t in outs)
    return (diff,) + tuple(t[:rows].cpu().numpy() for t in outs)


def post_frames(cols):
    """(name, entries, column that the network's arg-max is put on, row_correct at mask 1).  Weights are float32 multiples of 2^-10."""
    rng = np.random.RandomState(cols)
    frames = []

    def filler(n, banned, lo=0.0, hi=1.0, pool=None):
        pool = np.array([c for c in (pool if pool is not None else range(cols)) if c not in banned])
        return [(int(p), float(np.float32(np.round((lo + (hi - lo) * u) * 1024) / 1024))) for p, u in zip(pool[rng.randint(0, len(pool), n)], rng.rand(n))]

    frames.append(("empty", [], 0, 1))                              # the dense target row is all zero: its arg-max is column 0
    frames.append(("empty, network elsewhere", [], 5, 0))
    for n in (1, 255, 256, 257, 300, 600):
        for at in sorted({0, 255, 256, n - 1}):
            if at >= n:
                continue
            h = int(rng.randint(3, cols))
            fr = filler(n, {h})
            fr[at] = (h, 700.0)                                  # (600 fillers below 1 on one pdf stay below it)
            frames.append((f"{n} entries, heaviest first at {at}", fr, h, 1))
            if at >= 256:                                        # the best of the first 256 entries is where the network points: not correct
                first = fr[:256]
                acc = {}
                for p, w_ in fr:
                    acc[p] = acc.get(p, 0.0) + w_
                decoy = max({p for p, _ in first}, key=lambda p: (acc[p], -p))
                frames.append((f"{n} entries, heaviest first at {at}, network on the best of the first 256", fr, decoy, 0))
    for n, occ in ((300, (250, 260)), (600, (256, 300)), (600, (10, 599))):
        h, other = 7, 9
        fr = filler(n, {h, other}, hi=0.5)
        fr[5] = (other, 50.0)
        for e in occ:
            fr[e] = (h, 30.0)                                    # 30 + 30 beats 50 only as a sum
        frames.append((f"{n} entries, repeated pdf at {occ}", fr, h, 1))
    for n in (200, 300, 600):                                    # nothing positive; pdfs 0, 1, 2 present (late): the lowest implicit zero, 3, decides
        fr = filler(n, {0, 1, 2, 3}, lo=-1.0, hi=0.0)
        for e, p in zip((n - 40, n - 30, n - 20), (0, 1, 2)):
            fr[e] = (p, -0.5)
        frames.append((f"{n} entries <= 0, implicit zero at 3", fr, 3, 1))
        fr2 = list(fr)
        fr2[n - 10], fr2[n - 5] = (0, 0.25), (0, 0.25)           # pdf 0 sums to exactly zero: an explicit zero at 0
        frames.append((f"{n} entries <= 0, pdf 0 cancels to zero", fr2, 0, 1))
        frames.append((f"{n} entries <= 0, network not on the zero", fr, 1, 0))
    if cols <= 64:
        for n in (cols, 300, 600):                               # every pdf present and negative: no implicit zero
            w = -1.0 - rng.randint(0, 1024, cols) / 1024.0
            best = int(np.argmax(w))
            fr = [(e % cols, float(np.float32(w[e % cols])) if e < cols else 0.0) for e in range(n)]
            frames.append((f"{n} entries, all {cols} pdfs present and negative", fr, best, 1))
    if cols > 600:
        # columns 0 .. 255 (0 .. 299) all carry weight: the lowest zero is the first candidate of the SECOND round of the workgroup's zero
        # search (lies in the middle of it), so the search goes round its loop and through its pair of barriers again
        for n, span in ((600, 256), (600, 300), (257, 256)):
            fr = [(e % span, -1.0 - (e % 7) / 8.0) for e in range(n)]
            frames.append((f"{n} entries <= 0 on every column below {span}", fr, span, 1))
            frames.append((f"{n} entries <= 0 on every column below {span}, network on column 0", fr, 0, 0))
    # frames whose mask is not 1 are never correct: copies of frames that are correct at mask 1 (MASKS, by name)
    for name, fr, col, _ in [f for f in frames if f[0] in ("600 entries, heaviest first at 599", "300 entries <= 0, implicit zero at 3")]:
        for m in MASKS.values():
            frames.append((f"{name}, mask {m}", fr, col, 1))
    return frames


MASKS = {", mask 0.5": 0.5, ", mask 0.0": 0.0}


def post_calls(cols):
    """the frames of post_frames in calls of <= 8 rows: (frames, y, post, mask, the device's diff, row_xent, row_ent, row_correct)"""
    frames = post_frames(cols)
    base = R.softmax32(R.logits("trained", len(frames), cols, seed=5))
    for b in range(0, len(frames), 8):
        part = frames[b:b + 8]
        y = base[b:b + len(part)].copy()
        for r, (_, _, col, _) in enumerate(part):
            m = y[r].argmax()
            y[r, [col, m]] = y[r, [m, col]]
        post = [fr for _, fr, _, _ in part]
        mask = np.array([next((m for suffix, m in MASKS.items() if name.endswith(suffix)), 1.0) for name, _, _, _ in part], np.float32)
        yield (part, y, post, mask) + gpu_post(y, post, mask)


@pytest.mark.parametrize("cols", (37, 4203))
def test_xent_post_any_number_of_entries(cols):
    """klstm_xent_eval_masked_post on frames of 0, 1, 255, 256, 257, 300 and 600 entries: the kernel stages 256 entries of a frame in LDS,
    and what lies past them has to count all the same -- the heaviest pdf first occurring at entry 0, 255, 256 or last, a repeated pdf
    across entry 256, no positive weight at all (the lowest zero of the dense row decides, implicit or cancelled; behind 256 or 300 occupied
    columns it lies in the second round of the workgroup's search), every pdf present, and copies at mask 0.5 and 0 of frames that are correct at 1.
    diff bit-equal to the dense float32 restatement (the additions run in the same order), row_correct exact against the oracle."""
    wrong, total = [], 0
    for part, y, post, mask, diff, _, _, rc in post_calls(cols):
        assert same_bits(diff, R.xent_post32(y, post, mask)[0]), [n for n, _, _, _ in part]
        correct = R.xent_post64(y, post, mask)[2]
        for r, (name, fr, col, expect) in enumerate(part):
            want = oc.xent_eval_masked_post(y[r:r + 1], [fr], mask[r:r + 1])[3]
            assert want == correct[r] == (expect if mask[r] == 1 else 0), name      # (the case is what its name says)
            total += 1
            if rc[r] != want:
                wrong.append((name, float(rc[r]), want))
    print(f"row_correct wrong in {len(wrong)} of {total} frames: {wrong}", flush=True)
    assert not wrong, wrong


@pytest.mark.parametrize("cols", (37, 4203))
def test_xent_post_entropies(cols):
    """cross entropy and target entropy of the same frames per row against float64: relative error at most max(4 x twin, 2^-21), both
    errors the largest over the frames.  A frame without a positive weight has the reference's NaN as its target entropy (log of a
    negative number, nnet-loss.cc:130-136) and must return it.
    MEASURED.  37 columns: cross entropy 1.48e-07 (twin 1.49e-07, bar 5.97e-07), target entropy 9.2e-08 (twin 2.20e-07, bar 8.82e-07).
    4203 columns: cross entropy 1.08e-07 (twin 1.10e-07, bar 4.77e-07), target entropy 1.79e-07 (twin 3.46e-07, bar 1.38e-06).
    The frame to watch is the one of 256 distinct pdfs at 4203 columns: every thread holds one term, and the kernel adds the 256 in double
    (one float32 accumulator gives 5.03e-07 there)."""
    figs = []
    for part, y, post, mask, _, xe, en, _ in post_calls(cols):
        _, xe32, en32 = R.xent_post32(y, post, mask)
        xe64, en64, _ = R.xent_post64(y, post, mask)
        for r, (name, _, _, _) in enumerate(part):
            row = slice(r, r + 1)
            f = [("cross entropy", R.scalar_rel(xe[row], xe64[row]), R.scalar_rel(xe32[row], xe64[row]), FLOOR),
                 ("target entropy", R.scalar_rel(en[row], en64[row]), R.scalar_rel(en32[row], en64[row]), FLOOR)]
            print(f"{cols} columns, {name}: " + ", ".join(f"{w} {e:.3g} (twin {t:.3g})" for w, e, t, _ in f), flush=True)
            figs += f
    settle(figs, f"{cols} columns:")


# ---- the products ----
@functools.lru_cache(maxsize=None)
def engine():
    return k.Engine(40, 64, 32, 4)


def with_option(name, fn, f16):
    """fn(on, floor) -> the product as numpy, with the option on and off; the default (1) is back afterwards.  f16: the restated dispatch
    predicate (below) says that the f16 x 2 kernel serves this call when the option is on.  The floor follows the KERNEL: 2^-21 on two
    fp16 planes per operand, 2^-22 on every fp32 kernel, whatever the option says.  And because the two kinds of kernel round differently,
    the option must change the bits of the result exactly where the predicate says so: an `on` run that went to an fp32 kernel after
    all, or an fp32 shape that found its way onto fp16 planes, fails here."""
    e, got = engine(), {}
    try:
        for on in (1, 0):
            e.set_option(name, on)
            got[on] = fn(on, 2.0 ** -21 if on and f16 else 2.0 ** -22)
    finally:
        e.set_option(name, 1)
    assert same_bits(got[1], got[0]) == (not f16), f"{name}: the f16 x 2 kernel {'did not run' if f16 else 'ran'}, against the predicate"


# the dispatch of the stateless affine entries, restated (klstm_api_ops.hip; WINDOW / contiguous operands: strides % 4 == 0 with the widths)
def propagate_f16(rows, in_dim, out_dim, xlay):
    """direct_nt_supported, and inside launch_direct_nt the wide result with A shared through LDS (k_nt_shared_a16); the narrow results
    (k_direct_nt_ks: out_dim <= 8192 and in_dim % 512 == 0) and k_direct_nt are fp32"""
    return aligned(xlay) and 1 <= rows <= 80 and in_dim % 128 == 0 and out_dim > 8192 and in_dim % 256 == 0


def backpropagate_f16(rows, in_dim, out_dim):
    """skinny_nn_supported's first line (k_skinny_nn16); k_skinny_nn, the split-K and the tiled kernel are fp32"""
    return 1 <= rows <= 80 and in_dim % 4 == 0 and 64 <= in_dim <= 1024 and out_dim >= 4096 and out_dim % 8 == 0


def outer_f16(rows, in_dim, out_dim):
    """outer_f16_supported (the bias of klstm_affine_update is not part of it: only bias_corr has to be aligned)"""
    return 1 <= rows <= 96 and out_dim >= 2048 and out_dim % 4 == 0 and in_dim >= 64 and in_dim % 4 == 0


@functools.lru_cache(maxsize=8)
def derivatives(rows, cols):
    """(y - onehot) * mask of trained posteriors, some rows masked"""
    a = R.logits("trained", rows, cols, seed=6)
    y = R.softmax32(a)
    target = np.random.RandomState(rows + cols).randint(0, cols, rows).astype(np.int32)
    mask = (np.random.RandomState(rows).rand(rows) > 0.2).astype(np.float32)
    d = R.diff32(y, target, mask)
    d.setflags(write=False)
    return d


def operands(rows, in_dim, out_dim):
    rng = np.random.RandomState(rows + 3 * in_dim + 7 * out_dim)
    x = rng.uniform(-1, 1, (rows, in_dim)).astype(np.float32)
    W = (0.2 * rng.randn(out_dim, in_dim)).astype(np.float32)
    b = rng.uniform(-12, -4, out_dim).astype(np.float32)
    return x, W, b


def comp_err(C, ref, den):
    d = np.abs(C.astype(np.float64) - ref)
    assert not d[den == 0].any()
    return float((d[den > 0] / den[den > 0]).max())


PROP = [(16, 512, 8208), (17, 512, 8208), (80, 512, 8208), (81, 512, 8208), (80, 100, 8208), (80, 128, 8208), (80, 384, 8208),
        (80, 512, 60), (80, 512, 64), (80, 512, 8192), (80, 128, 8192), (80, 512, 8201), (80, 384, 8201), (80, 512, 16384), (80, 512, 16400),
        (17, 128, 64), (81, 100, 60), (16, 384, 16384)]


@pytest.mark.parametrize("rows,in_dim,out_dim,xlay", [s + (WINDOW,) for s in PROP] + [(80, 512, 8208, OFF1), (80, 512, 16400, ODD)])
def test_affine_propagate_componentwise(rows, in_dim, out_dim, xlay):
    """out = x W^T + bias on both sides of what klstm_affine_propagate's dispatch reads (rows 80 / 81, in_dim % 128, out_dim 64 and 8192,
    an odd width, a misaligned or odd-strided input), |out - out64| / (|x| |W|^T + |bias|) per element"""
    x, W, b = operands(rows, in_dim, out_dim)
    x64, W64, b64 = x.astype(np.float64), W.astype(np.float64), b.astype(np.float64)
    ref, den = x64 @ W64.T + b64, np.abs(x64) @ np.abs(W64).T + np.abs(b64)
    e32 = comp_err(x @ W.T + b, ref, den)
    xin, Wd, bd = Buf(rows, in_dim, xlay, x), f32(W), f32(b)

    def run(on, floor):
        out = Buf(rows, out_dim, WINDOW)
        k.affine_propagate(xin.v, Wd, bd, out.v)
        got = out.get()
        err = comp_err(got, ref, den)
        print(f"propagate {rows}x{in_dim}x{out_dim} fp16_products={on}: {err:.3g} (numpy float32 {e32:.3g}, floor {floor:.3g})", flush=True)
        bound(err, max(4 * e32, floor), f"out, fp16_products={on}")
        xin.get()
        return got
    with_option("fp16_products", run, propagate_f16(rows, in_dim, out_dim, xlay))


@pytest.mark.parametrize("rows", (80, 81))
@pytest.mark.parametrize("in_dim", (60, 64, 1024, 1028))
@pytest.mark.parametrize("out_dim", (4088, 4096, 4100, 4104))
def test_affine_backpropagate_componentwise(rows, in_dim, out_dim):
    """in_diff = out_diff W around skinny_nn_supported (<= 80 rows, out_dim >= 4096 and % 8, in_dim 64 ... 1024) and the split-K plan"""
    _, W, _ = operands(rows, in_dim, out_dim)
    d = derivatives(rows, out_dim)
    d64, W64 = d.astype(np.float64), W.astype(np.float64)
    ref, den = d64 @ W64, np.abs(d64) @ np.abs(W64)
    e32 = comp_err(d @ W, ref, den)
    din, Wd = Buf(rows, out_dim, WINDOW, d), f32(W)

    def run(on, floor):
        ind = Buf(rows, in_dim, WINDOW)
        k.affine_backpropagate(din.v, Wd, ind.v)
        got = ind.get()
        err = comp_err(got, ref, den)
        print(f"backpropagate {rows}x{in_dim}x{out_dim} skinny_f16={on}: {err:.3g} (numpy float32 {e32:.3g}, floor {floor:.3g})", flush=True)
        bound(err, max(4 * e32, floor), f"in_diff, skinny_f16={on}")
        din.get()
        return got
    with_option("skinny_f16", run, backpropagate_f16(rows, in_dim, out_dim))


# out_dim "ride" = 64 n + n and "past" = 64 n + n + 4 for the device's n compute units: the rows past the last whole strip per unit ride
# along with the strips / start a round of their own (klstm_outer.hip)
OUTER = [(r, 512, m) for r in (32, 33, 64, 65, 96, 97) for m in (2048, "ride")] + \
        [(r, 512, m) for r in (96, 97) for m in (2044, "past")] + [(33, 128, 2044), (64, 128, "past")]


def outer_dim(m):
    n = torch.cuda.get_device_properties(0).multi_processor_count
    return {"ride": 64 * n + n, "past": 64 * n + n + 4}.get(m, m)


LR, LR_B, MMT = 0.02, 0.05, 0.9


@pytest.mark.parametrize("rows,in_dim,out_dim", OUTER)
def test_affine_gradient_componentwise(rows, in_dim, out_dim):
    """W_grad = out_diff^T x, bias_grad = column sums, around outer_f16_supported (<= 96 rows, out_dim >= 2048) and the width at which the
    rows past the last whole strip per compute unit ride along or do not"""
    check_gradient(rows, in_dim, outer_dim(out_dim))


@pytest.mark.parametrize("rows,in_dim,out_dim", OUTER)
def test_affine_update_componentwise(rows, in_dim, out_dim):
    """klstm_affine_update twice (the second call has momentum to apply): W_corr, bias_corr and the parameter changes theta - theta_0"""
    check_update(rows, in_dim, outer_dim(out_dim))


@pytest.mark.parametrize("rows,in_dim,out_dim", [(64, 102, 2048), (97, 102, 2048), (33, 30, 257)])
def test_affine_gradient_odd_in_dim(rows, in_dim, out_dim):
    """in_dim % 4 != 0: the tiled product (launch_gemm) instead of the coalesced one, and no f16 x 2 kernel"""
    check_gradient(rows, in_dim, out_dim)


@pytest.mark.parametrize("rows,in_dim,out_dim,bias_off", [(64, 102, 2048, 0), (97, 102, 2048, 0), (33, 30, 257, 0),     # launch_gemm + launch_axpy
                                                          (64, 128, 2048, 1), (96, 512, 2052, 1)])                        # bias one float in
def test_affine_update_unreached_branches(rows, in_dim, out_dim, bias_off):
    """klstm_affine_update with in_dim % 4 != 0 (the product and the parameter step as two launches) and with a bias that is not 16-byte
    aligned (its step beside launch_outer_f16 instead of inside it)"""
    check_update(rows, in_dim, out_dim, bias_off)


def check_gradient(rows, in_dim, out_dim):
    x, _, _ = operands(rows, in_dim, out_dim)
    d = derivatives(rows, out_dim)
    d64, x64 = d.astype(np.float64), x.astype(np.float64)
    ref, den = d64.T @ x64, np.abs(d64).T @ np.abs(x64)
    bref, bden = d64.sum(0), np.abs(d64).sum(0)
    e32, b32 = comp_err(d.T @ x, ref, den), comp_err(d.sum(0, dtype=np.float32), bref, bden)
    pad = WINDOW if in_dim % 4 == 0 else ODD
    xin, din = Buf(rows, in_dim, pad, x), Buf(rows, out_dim, WINDOW, d)

    def run(on, floor):
        gW = torch.full((out_dim + 1, in_dim), SENT, device="cuda")
        gb = torch.full((out_dim + 1,), SENT, device="cuda")
        k.affine_gradient(xin.v, din.v, gW[:out_dim], gb[:out_dim])
        torch.cuda.synchronize()
        assert bool((gW[out_dim] == SENT).all()) and gb[out_dim].item() == SENT
        got = gW[:out_dim].cpu().numpy()
        err, berr = comp_err(got, ref, den), comp_err(gb[:out_dim].cpu().numpy(), bref, bden)
        print(f"gradient {rows}x{in_dim}x{out_dim} outer_f16={on}: W_grad {err:.3g} (numpy float32 {e32:.3g}, floor {floor:.3g}) "
              f"bias_grad {berr:.3g} ({b32:.3g})", flush=True)
        bound(err, max(4 * e32, floor), f"W_grad {rows}x{in_dim}x{out_dim}, outer_f16={on}")
        bound(berr, max(4 * b32, 2.0 ** -22), f"bias_grad {rows}x{in_dim}x{out_dim}, outer_f16={on}")
        xin.get(); din.get()
        return got
    with_option("outer_f16", run, outer_f16(rows, in_dim, out_dim))


def check_update(rows, in_dim, out_dim, bias_off=0):
    x, W, b = operands(rows, in_dim, out_dim)
    d = derivatives(rows, out_dim)
    d64, x64 = d.astype(np.float64), x.astype(np.float64)
    g, gden = d64.T @ x64, np.abs(d64).T @ np.abs(x64)
    gb, gbden = d64.sum(0), np.abs(d64).sum(0)
    # two calls from zero momentum: corr = (1 + m) g, theta - theta_0 = -lr (2 + m) g; the parameters' own rounding belongs to the denominator
    lr, lrb, m = (float(np.float32(v)) for v in (LR, LR_B, MMT))
    truth = dict(W_corr=((1 + m) * g, (1 + m) * gden), bias_corr=((1 + m) * gb, (1 + m) * gbden),
                 dW=(-lr * (2 + m) * g, lr * (2 + m) * gden + np.abs(W.astype(np.float64))),
                 dbias=(-lrb * (2 + m) * gb, lrb * (2 + m) * gbden + np.abs(b.astype(np.float64))))
    W2, b2, Wc, bc = W.copy(), b.copy(), np.zeros_like(W), np.zeros_like(b)
    for _ in range(2):
        oc.affine_update(x, d, W2, b2, Wc, bc, np.float32(LR), np.float32(LR_B), np.float32(MMT))
    twin = dict(W_corr=Wc, bias_corr=bc, dW=W2.astype(np.float64) - W, dbias=b2.astype(np.float64) - b)
    e32 = {n: comp_err(twin[n], *truth[n]) for n in truth}
    pad = WINDOW if in_dim % 4 == 0 else ODD
    xin, din = Buf(rows, in_dim, pad, x), Buf(rows, out_dim, WINDOW, d)

    def run(on, floor):
        Wd = torch.full((out_dim + 1, in_dim), SENT, device="cuda"); Wd[:out_dim] = f32(W)
        Wcd = torch.full((out_dim + 1, in_dim), SENT, device="cuda"); Wcd[:out_dim] = 0
        bd = torch.full((out_dim + 8,), SENT, device="cuda"); bv = bd[bias_off:bias_off + out_dim]; bv.copy_(f32(b))
        bcd = torch.full((out_dim + 4,), SENT, device="cuda"); bcd[:out_dim] = 0
        for _ in range(2):
            k.affine_update(xin.v, din.v, Wd[:out_dim], bv, Wcd[:out_dim], bcd[:out_dim], LR, LR_B, MMT)
        torch.cuda.synchronize()
        assert bool((Wd[out_dim] == SENT).all()) and bool((Wcd[out_dim] == SENT).all()) and bool((bcd[out_dim:] == SENT).all())
        assert bool((bd[:bias_off] == SENT).all()) and bool((bd[bias_off + out_dim:] == SENT).all())
        got = dict(W_corr=Wcd[:out_dim].cpu().numpy(), bias_corr=bcd[:out_dim].cpu().numpy(),
                   dW=Wd[:out_dim].cpu().numpy().astype(np.float64) - W, dbias=bv.cpu().numpy().astype(np.float64) - b)
        errs = {n: comp_err(got[n], *truth[n]) for n in truth}
        print(f"update {rows}x{in_dim}x{out_dim} bias+{bias_off} outer_f16={on}: " +
              " ".join(f"{n} {errs[n]:.3g} (numpy float32 {e32[n]:.3g})" for n in truth) + f" (floor of the products {floor:.3g})", flush=True)
        for n in truth:
            bound(errs[n], max(4 * e32[n], floor if n in ("W_corr", "dW") else 2.0 ** -22), f"{n} {rows}x{in_dim}x{out_dim}, outer_f16={on}")
        xin.get(); din.get()
        return got["W_corr"]
    with_option("outer_f16", run, outer_f16(rows, in_dim, out_dim))
