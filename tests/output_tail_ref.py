"""Truths and twins of the output layer (AffineTransform, Softmax, Xent::EvalMasked, the scorer's log-softmax), plain numpy.
truth64: the operation in float64 from the float32 inputs.  twin32: the kernels' RECIPE in numpy float32 with numpy's accurate exp / log --
subtract the row maximum, exp, float32 sum, multiply by 1 / sum; log forms as (a - max) - log(sum).  The twin is the yardstick of the GPU
tests (tests/test_output_tail_gpu.py: bar = max(4 x the twin's error, floor)); the kernel is never its own yardstick.
tests/test_output_tail.py pins this file against torch and oracle/components.py."""
import numpy as np

REGIMES = ("flat", "trained", "wide", "saturated")
TINY = 2.0 ** -102          # relative errors are taken over true values >= TINY: 24 binary orders above the float32 subnormals (2^-126)
TINY_OUT = 2.0 ** -101      # what an excluded element may come back as at most
POSTERIOR, LOGPOST, LOGLIKE = 0, 1, 2
F32 = np.float32


def logits(regime, rows, cols, seed=0):
    """float32 [rows, cols].  flat: 0.05 N(0,1).  trained: 3 N(0,1) with +12 on one column per row.  wide: uniform on [-60, 30], one draw
    per cell of width 90 / cols in shuffled order (so that the share of a short row below any level is the distribution's and not the
    luck of three draws).  saturated: trained with +200 instead of +12 (posteriors exactly 0.0 and 1.0 in float32)."""
    rng = np.random.RandomState(7919 * REGIMES.index(regime) + 104729 * seed + cols)
    if regime == "flat":
        return (0.05 * rng.randn(rows, cols)).astype(F32)
    if regime == "wide":
        a = np.empty((rows, cols))
        for r in range(rows):
            a[r] = -60.0 + 90.0 * (rng.permutation(cols) + rng.rand(cols)) / cols
        return a.astype(F32)
    a = 3.0 * rng.randn(rows, cols)
    a[np.arange(rows), rng.randint(0, cols, rows)] += 12.0 if regime == "trained" else 200.0
    return a.astype(F32)


# ---- truth64 ----
def log_softmax64(a):
    d = a.astype(np.float64) - a.astype(np.float64).max(1, keepdims=True)
    return d - np.log(np.exp(d).sum(1, keepdims=True))


def softmax64(a):
    d = a.astype(np.float64) - a.astype(np.float64).max(1, keepdims=True)
    e = np.exp(d)
    return e / e.sum(1, keepdims=True)


def score64(a, mode, log_prior=None, prior_scale=1.0):
    """the scorer's three outputs: posterior, log-posterior, log-posterior - prior_scale * log_prior"""
    if mode == POSTERIOR:
        return softmax64(a)
    v = log_softmax64(a)
    return v - float(F32(prior_scale)) * log_prior.astype(np.float64) if mode == LOGLIKE else v


def onehot(target, rows, cols, dtype):
    t = np.zeros((rows, cols), dtype)
    ok = (target >= 0) & (target < cols)                    # (an out-of-range target subtracts nothing)
    t[np.arange(rows)[ok], target[ok]] = 1
    return t


def argmax_first(y):
    return y.argmax(1)                                      # numpy: the first maximum, like FindRowMaxId


def xent64(y, target, mask):
    """Xent::EvalMasked for one-hot targets from the float32 posterior y: diff, row_xent = -mask * log(y[target]) (0 where the target
    is out of range), row_correct, valid frames"""
    rows, cols = y.shape
    ok = (target >= 0) & (target < cols)
    m = mask.astype(np.float64)
    diff = (y.astype(np.float64) - onehot(target, rows, cols, np.float64)) * m[:, None]
    yt = y[np.arange(rows), np.where(ok, target, 0)].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rx = np.where(ok, -m * np.log(yt), 0.0)
    correct = ((mask == 1) & (argmax_first(y) == target)).astype(np.float64)
    return diff, rx, correct, int(mask.sum())


def xent_from_logits64(a, target, mask):
    """row_xent of the one-pass kernel's contract: -mask * log softmax(a)[target], from the logits"""
    rows, cols = a.shape
    ok = (target >= 0) & (target < cols)
    ls = log_softmax64(a)[np.arange(rows), np.where(ok, target, 0)]
    return np.where(ok, -mask.astype(np.float64) * ls, 0.0)


def dense_target(post, rows, cols, dtype):
    """nnet-loss.cc:85-96: tgt(t, pdf) += weight in list order (dtype float32: the reference's own additions)"""
    t = np.zeros((rows, cols), dtype)
    for r, fr in enumerate(post):
        for pdf, w in fr:
            t[r, pdf] += dtype(F32(w))
    return t


def xent_post64(y, post, mask):
    """Xent::EvalMasked for general posteriors: row cross entropy -mask * sum t log y, row target entropy -mask * sum t log(t + 1e-20),
    row_correct (arg-max of the dense target, first maximum).  The sums run over the pdfs that occur: an absent pdf contributes t = 0."""
    rows, cols = y.shape
    t = dense_target(post, rows, cols, np.float64)
    m = mask.astype(np.float64)
    xe, en = np.zeros(rows), np.zeros(rows)
    with np.errstate(divide="ignore", invalid="ignore"):
        for r, fr in enumerate(post):
            pd = sorted({p for p, _ in fr})
            xe[r] = -(np.log(y[r, pd].astype(np.float64)) * t[r, pd]).sum() * m[r]
            en[r] = -(np.log(t[r, pd] + float(F32(1e-20))) * t[r, pd]).sum() * m[r]
    correct = ((mask == 1) & (argmax_first(y) == dense_target(post, rows, cols, F32).argmax(1))).astype(np.float64)
    return xe, en, correct


def targets_for(a):
    """the targets of the GPU tests' accuracy runs: the hot column on even rows, a seeded counted column on odd rows"""
    rows, cols = a.shape
    rng = np.random.RandomState(cols + 1)
    t = softmax64(a)
    tgt = t.argmax(1)
    for r in range(1, rows, 2):
        ok = np.flatnonzero(counted(t[r]))
        tgt[r] = ok[rng.randint(0, len(ok))]
    return tgt.astype(np.int32)


# ---- twin32 ----
def _parts32(a):
    d = a - a.max(1, keepdims=True)
    e = np.exp(d)
    s = e.sum(1, keepdims=True, dtype=F32)
    assert d.dtype == F32 and e.dtype == F32 and s.dtype == F32
    return d, e, s


def softmax32(a):
    _, e, s = _parts32(a)
    return e * (F32(1.0) / s)


def score32(a, mode, log_prior=None, prior_scale=1.0):
    d, e, s = _parts32(a)
    if mode == POSTERIOR:
        return e * (F32(1.0) / s)
    v = d - np.log(s)
    return v - F32(prior_scale) * log_prior if mode == LOGLIKE else v


def diff32(y, target, mask):
    """(y - onehot) * mask in float32: one subtraction and one product per element"""
    return (y - onehot(target, y.shape[0], y.shape[1], F32)) * mask[:, None]


def xent32(y, target, mask):
    rows, cols = y.shape
    ok = (target >= 0) & (target < cols)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ok, -mask * np.log(y[np.arange(rows), np.where(ok, target, 0)]), F32(0)).astype(F32)


def xent_post32(y, post, mask):
    """dense float32 restatement: diff (bit-exact contract: the additions run in list order), row cross entropy and entropy"""
    rows, cols = y.shape
    t = dense_target(post, rows, cols, F32)
    diff = (y - t) * mask[:, None]
    xe, en = np.zeros(rows, F32), np.zeros(rows, F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for r, fr in enumerate(post):
            pd = sorted({p for p, _ in fr})
            xe[r] = -((np.log(y[r, pd]) * t[r, pd]) * mask[r]).sum(dtype=F32)
            en[r] = -((np.log(t[r, pd] + F32(1e-20)) * t[r, pd]) * mask[r]).sum(dtype=F32)
    return diff, xe, en


# ---- measures ----
def counted(truth):
    """the elements a relative error is taken over"""
    return truth >= TINY


def rel_err(x, truth):
    """max |x - truth| / truth over the counted elements (posteriors)"""
    c = counted(truth)
    return float((np.abs(x.astype(np.float64) - truth)[c] / truth[c]).max()) if c.any() else 0.0


def log_err(x, truth):
    """max |x - truth| / max(1, |truth|) (log forms)"""
    return float((np.abs(x.astype(np.float64) - truth) / np.maximum(1.0, np.abs(truth))).max())


def scalar_rel(x, truth):
    """per element |x - truth| / |truth| (0 where both are 0, NaN must meet NaN), maximum"""
    x, truth = np.asarray(x, np.float64), np.asarray(truth, np.float64)
    same = (x == truth) | (np.isnan(x) & np.isnan(truth))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(same, 0.0, np.abs(x - truth) / np.abs(truth))
    return float(np.max(np.where(np.isnan(r), np.inf, r))) if r.size else 0.0


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(F32)).astype(np.float64)


def product_err(C, A64, B64):
    """componentwise error of a product: max_ij |C - A B|_ij / (|A| |B|)_ij, both from float64 (elements with a zero denominator
    must be exactly zero)"""
    ref, den = A64 @ B64, np.abs(A64) @ np.abs(B64)
    d = np.abs(C.astype(np.float64) - ref)
    assert not d[den == 0].any(), "a product of zeros is not zero"
    return float((d[den > 0] / den[den > 0]).max()) if (den > 0).any() else 0.0
