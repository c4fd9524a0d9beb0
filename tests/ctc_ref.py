"""Yardsticks of the CTC tests (tests/test_ctc.py, tests/test_ctc_gpu.py, tests/test_ctc_small.py, tests/test_ctc_small_gpu.py), host only:
  oracle()         torch.nn.functional.ctc_loss on the CPU in float64 (or float32: "stock fp32", the bar's yardstick), the exact recipe
                   the kernel's semantics were fixed against.  It is exact to ITS OWN input, log(clamp(y)) taken in float32 and then cast,
                   behind a log_softmax that renormalises every row whose float32 sum is not 1 -- which the kernel does not do.  So its
                   float64 loss is 6e-8 to 1.5e-7 (relative) away from the loss of the raw posteriors: nothing under the bars of
                   tests/test_ctc_gpu.py, too much for the bars of the small suite, which uses truth64()
  truth64()        loss and diff of the RAW float32 posteriors as the kernel defines them, float64 throughout: emissions
                   log(max(double(y), FLT_MIN)), no renormalisation, loss = -log sum_paths prod_t y, diff = y - gamma
  truth_core()     its per-utterance core on float64 posteriors taken as given: (log p, gamma)
  brute_force()    -log of the sum over ALL alignments, float64, for tiny cases: pins oracle() and truth64() independently of torch
  norm_twin()      the kernel's own recursion (normalised log domain, offsets summed in double) in numpy float32
  infeasible()     which streams klstm_ctc_eval must reject, from the lengths and labels alone
  single_path()    the one alignment of an exactly feasible utterance (len == L + repeats)
  make_case()      the seeded inputs of the parity cases: posteriors = fp32 softmax of scale * randn
  small_grid()     every label sequence of length 0..3 over the non-blank classes at every length 1..9, packed 32 streams to a call
  small_posteriors()  the posteriors of the small suite: flat, peaked, saturated (one-hot rows of exact 0.0 and 1.0)
  small_group()    the calls of one (K, blank, kind) group of the small suite with truth64 and norm_twin of every stream, computed once
  batch_twin()     the numpy twin of WholeUtteranceBatcher (include/klstm_trainer.hpp)"""
import functools
import itertools

import numpy as np
import torch
import torch.nn.functional as F

FLT_MIN = float(np.finfo(np.float32).tiny)
NEG = np.float32(-1e30)


def infeasible(lens, labels, K, blank, T=None):
    out = []
    for n, lab in zip(lens, labels):
        lab = list(lab)
        rep = sum(1 for a, b in zip(lab[:-1], lab[1:]) if a == b)
        bad = any(c < 0 or c >= K or c == blank for c in lab)
        out.append(n > 0 and (n < len(lab) + rep or bad or (T is not None and n > T)))
    return out


def oracle(y, lens, labels, blank, dtype=torch.float64):
    """y [T, S, K] float32 posteriors.  Returns (loss [S] float64 numpy, diff [T, S, K] numpy of `dtype`); the diff is meaningful on the
    valid rows of feasible streams.  Idle streams (len 0) are left out of the torch call and come back as loss 0, diff 0."""
    y = torch.as_tensor(y, dtype=torch.float32)
    T, S, K = y.shape
    act = [s for s in range(S) if lens[s] > 0]
    loss = np.zeros(S)
    diff = np.zeros((T, S, K), dtype=np.float64 if dtype == torch.float64 else np.float32)
    if not act:
        return loss, diff
    a = torch.log(torch.clamp_min(y[:, act], FLT_MIN)).to(dtype).requires_grad_()
    flat = torch.tensor([c for s in act for c in labels[s]], dtype=torch.long)
    l = F.ctc_loss(F.log_softmax(a, -1), flat, torch.tensor([lens[s] for s in act]), torch.tensor([len(labels[s]) for s in act]),
                   blank=blank, reduction="none", zero_infinity=True)
    l.sum().backward()
    loss[act] = l.detach().double().numpy()
    diff[:, act] = a.grad.numpy()
    return loss, diff


def brute_force(y, labels, blank):
    """-log sum over all T-frame alignments that collapse to `labels` of prod_t y[t, path[t]]; y [T, K] float64."""
    T, K = y.shape
    tot = 0.0
    for path in itertools.product(range(K), repeat=T):
        col = [k for k, _ in itertools.groupby(path)]
        if [k for k in col if k != blank] == list(labels):
            tot += float(np.prod([y[t, path[t]] for t in range(T)]))
    return -np.log(tot) if tot > 0 else np.inf


def _lattice(lab, blank):
    """(extended label sequence [2L+1], skip [2L+1]: state i may be entered from i - 2)"""
    L = len(lab)
    ext = np.full(2 * L + 1, blank, dtype=np.int64)
    ext[1::2] = lab
    skip = np.zeros(2 * L + 1, dtype=bool)
    skip[3::2] = np.asarray(lab[1:]) != np.asarray(lab[:-1])
    return ext, skip


def truth_core(yd, lab, blank):
    """one feasible utterance, yd [n, K] FLOAT64 posteriors taken as given (valid frames only, clamped at FLT_MIN, not renormalised)
    -> (log p, gamma [n, K]) in float64, log domain throughout.  The core of truth64(), and of tests/ctc_mbr_ref.objective64()"""
    yd = np.asarray(yd, dtype=np.float64)
    n, K = yd.shape
    ext, skip = _lattice(lab, blank)
    N = ext.size
    em = np.log(np.maximum(yd, FLT_MIN))[:, ext]                            # [n, N]
    ninf = np.full(2, -np.inf)
    A = np.full((n, N), -np.inf)
    B = np.full((n, N), -np.inf)
    A[0, :2] = em[0, :2]
    B[n - 1, max(N - 2, 0):] = 0.0
    skip_b = np.concatenate([skip[2:], [False, False]])[:N]                 # state i may leave for i + 2
    with np.errstate(invalid="ignore"):                                     # logaddexp(-inf, -inf) = -inf
        for t in range(1, n):
            p = np.concatenate([ninf, A[t - 1]])
            A[t] = np.logaddexp(np.logaddexp(p[2:], p[1:-1]), np.where(skip, p[:-2], -np.inf)) + em[t]
        for t in range(n - 2, -1, -1):
            p = np.concatenate([B[t + 1] + em[t + 1], ninf])
            B[t] = np.logaddexp(np.logaddexp(p[:-2], p[1:-1]), np.where(skip_b, p[2:], -np.inf))
        logp = np.logaddexp.reduce(A[n - 1, max(N - 2, 0):])
        g = A + B
        m = g.max(1, keepdims=True)
        g = g - (m + np.log(np.exp(g - m).sum(1, keepdims=True)))           # per frame: log sum_i alpha beta = log p on every frame
    gam = np.zeros((n, K))
    np.add.at(gam, (np.arange(n)[:, None], ext[None, :]), np.exp(g))
    return logp, gam


def _truth_one(y, lab, blank):
    """one feasible utterance, y [n, K] float32 (valid frames only) -> (loss, diff [n, K]) in float64"""
    yd = np.asarray(y, dtype=np.float32).astype(np.float64)
    logp, gam = truth_core(yd, lab, blank)
    return float(-logp), yd - gam


def truth64(y, lens, labels, blank):
    """y [T, S, K] float32 posteriors.  Returns (loss [S], diff [T, S, K]) in float64 of the RAW posteriors as klstm_ctc_eval defines
    them: emissions log(max(double(y), FLT_MIN)) taken in double, no renormalisation of the rows, loss = -log sum_paths prod_t y,
    diff = y - gamma; a direct log-domain forward-backward (the linear domain would underflow: FLT_MIN ** 9 is no double).  Idle
    streams: loss 0; infeasible ones: loss +inf; both with diff 0, as are the padding rows."""
    y = torch.as_tensor(y, dtype=torch.float32).numpy()
    T, S, K = y.shape
    bad = infeasible(lens, labels, K, blank, T)
    loss, diff = np.zeros(S), np.zeros((T, S, K))
    for s in range(S):
        n = lens[s]
        if n == 0:
            continue
        if bad[s]:
            loss[s] = np.inf
            continue
        loss[s], diff[:n, s] = _truth_one(y[:n, s], list(labels[s]), blank)
    return loss, diff


def single_path(lab, blank):
    """the only alignment of `lab` to len(lab) + repeats frames: the labels in order, one blank between two equal neighbours"""
    path = []
    for j, c in enumerate(lab):
        if j and lab[j - 1] == c:
            path.append(blank)
        path.append(c)
    return path


def _lse3(x0, x1, x2):
    m = np.maximum(x0, np.maximum(x1, x2))
    return m + np.log(np.exp(x0 - m) + np.exp(x1 - m) + np.exp(x2 - m), dtype=np.float32)


def norm_twin(y, lab, blank):
    """One utterance, y [T, K] float32 (valid frames only).  Returns (loss float, diff [T, K] float32) by the kernel's recipe: the row of
    step u is taken relative to the maximum of the row before it; alpha includes the frame's emission, beta does not."""
    y = np.asarray(y, dtype=np.float32)
    T, K = y.shape
    L = len(lab)
    N = 2 * L + 1
    ext = np.full(N, blank, dtype=np.int64)
    ext[1::2] = lab
    skip = np.zeros(N, dtype=bool)
    skip[3::2] = np.asarray(lab[1:]) != np.asarray(lab[:-1])
    em = np.log(np.maximum(y, np.float32(FLT_MIN)))[:, ext]                 # [T, N] float32
    A = np.empty((T, N), np.float32)
    B = np.empty((T, N), np.float32)
    csum = 0.0
    for d in (0, 1):
        w = None
        for u in range(T):
            tt = T - 1 - u if d else u
            if u == 0:
                base = np.full(N, NEG, np.float32)
                if d:
                    base[max(N - 2, 0):] = 0
                else:
                    base[:2] = 0
            else:
                M = w.max()
                if d == 0:
                    csum += float(M)
                pad = np.concatenate([[NEG, NEG], w, [NEG, NEG]]).astype(np.float32)
                if d:
                    x1, x2 = pad[3:3 + N], np.where(np.concatenate([skip[2:], [False, False]])[:N], pad[4:4 + N], NEG)
                else:
                    x1, x2 = pad[1:1 + N], np.where(skip, pad[0:N], NEG)
                base = (_lse3(w, x1, x2.astype(np.float32)) - M).astype(np.float32)
            w = (base + em[tt]).astype(np.float32)
            (B if d else A)[tt] = base if d else w
            if d == 0 and u == T - 1:
                tail = w[max(N - 2, 0):]
                loss = -(csum + float(tail.max() + np.log(np.exp(tail - tail.max()).sum(dtype=np.float32))))
    g = A + B
    e = np.exp(g - g.max(1, keepdims=True))
    gam = np.zeros((T, K), np.float32)
    np.add.at(gam, (np.arange(T)[:, None], ext[None, :]), e / e.sum(1, keepdims=True, dtype=np.float32))
    return loss, y - gam


def make_case(seed, T, K, scale, lens, lab_lens, blank=0, equal_labels=()):
    """posteriors [T, S, K] float32 = softmax(scale * randn); random labels != blank; streams in `equal_labels` repeat one class."""
    g = torch.Generator().manual_seed(seed)
    S = len(lens)
    y = torch.softmax(torch.randn(T, S, K, generator=g) * scale, -1)
    labels = []
    for s, n in enumerate(lab_lens):
        lab = torch.randint(0, K - 1, (n,), generator=g)
        lab = lab + (lab >= blank).long()                   # skips the blank
        if s in equal_labels and n:
            lab = torch.full((n,), int(lab[0]))
        labels.append(lab.tolist())
    return y, labels


SMALL_T, SMALL_S = 9, 32           # the block of a call of the small suite: frames, streams (one of them idle)


def small_grid(K, blank):
    """Every label sequence of length 0..3 over the non-blank classes of K, at every length 1..SMALL_T: 15 * 9 = 135 utterances at K = 3,
    36 at K = 2, 360 at K = 4, about a quarter of them infeasible.  Yields (lens, labels) of one call each: up to 31 utterances (the
    lengths cycle fastest, so a call mixes them and has padding rows under the block's T = 9) and one idle stream (len 0, no labels)
    planted at a position that moves from call to call."""
    classes = [c for c in range(K) if c != blank]
    utts = [(n, list(lab)) for L in range(4) for lab in itertools.product(classes, repeat=L) for n in range(1, SMALL_T + 1)]
    for call, b in enumerate(range(0, len(utts), SMALL_S - 1)):
        part = utts[b:b + SMALL_S - 1]
        part.insert((7 * call + 3) % (len(part) + 1), (0, []))
        yield [n for n, _ in part], [lab for _, lab in part]


def small_posteriors(kind, T, S, K, generator):
    """[T, S, K] float32.  flat: softmax(randn); peaked: softmax(8 randn); saturated: one-hot rows of exact 0.0 and 1.0, the hot class
    uniform -- what a saturated softmax delivers, so that many feasible labellings run through clamped zeros."""
    if kind == "saturated":
        return F.one_hot(torch.randint(0, K, (T, S), generator=generator), K).float()
    return torch.softmax(torch.randn(T, S, K, generator=generator) * {"flat": 1.0, "peaked": 8.0}[kind], -1)


SMALL_GROUPS = [(3, 0), (3, 1), (3, 2), (2, 0), (2, 1), (4, 0), (4, 3)]     # (K, blank); K = 4: the float4 path of k_ctc_combine
SMALL_KINDS = ["flat", "peaked", "saturated"]


def twin_batch(y, lens, labels, blank, bad):
    """norm_twin over the feasible streams of a call -> (loss [S] float64 as norm_twin returns it, diff [T, S, K] float32), zero elsewhere"""
    y = torch.as_tensor(y).numpy()
    T, S, K = y.shape
    loss, diff = np.zeros(S), np.zeros((T, S, K), np.float32)
    for s in range(S):
        if lens[s] > 0 and not bad[s]:
            loss[s], diff[:lens[s], s] = norm_twin(y[:lens[s], s], list(labels[s]), blank)
    return loss, diff


def pooled_errors(loss, diff, l64, d64, lens, bad):
    """(max |diff - truth| over the valid rows, max |loss - truth| / max(1, |truth|)) pooled over the feasible streams of a call"""
    e = r = 0.0
    for s, n in enumerate(lens):
        if n > 0 and not bad[s]:
            e = max(e, float(np.abs(diff[:n, s].astype(np.float64) - d64[:n, s]).max()))
            r = max(r, abs(float(loss[s]) - l64[s]) / max(1.0, abs(l64[s])))
    return e, r


@functools.lru_cache(maxsize=None)
def small_group(K, blank, kind, seed=7):
    """the calls of one group of the small suite, each a dict(y [T, S, K], lens, labels, bad (infeasible()), l64, d64 (truth64), ltw,
    dtw (twin_batch)); computed once per session and shared: nothing may modify it"""
    g = torch.Generator().manual_seed(seed)
    calls = []
    for lens, labels in small_grid(K, blank):
        y = small_posteriors(kind, SMALL_T, len(lens), K, g)
        bad = infeasible(lens, labels, K, blank, SMALL_T)
        l64, d64 = truth64(y, lens, labels, blank)
        ltw, dtw = twin_batch(y, lens, labels, blank, bad)
        calls.append(dict(y=y, lens=lens, labels=labels, bad=bad, l64=l64, d64=d64, ltw=ltw, dtw=dtw))
    return calls


def batch_twin(utts, S, sort, max_frames):
    """utts: list of (feats [n, dim], labels).  Returns (minibatches, skipped): each minibatch = dict(T, feat [T*S, dim], lens [S],
    labels [S lists], index [S] utterance numbers or -1)."""
    order = [i for i, (f, _) in enumerate(utts) if len(f) <= max_frames and len(f) > 0]
    skipped = len(utts) - len(order)
    if sort:
        order = sorted(order, key=lambda i: -len(utts[i][0]))        # stable
    out = []
    for b in range(0, len(order), S):
        ids = order[b:b + S]
        T = max(len(utts[i][0]) for i in ids)
        dim = utts[ids[0]][0].shape[1]
        feat = np.zeros((T * S, dim), np.float32)
        lens, labels, index = [0] * S, [[] for _ in range(S)], [-1] * S
        for s, i in enumerate(ids):
            f, lab = utts[i]
            feat[s:len(f) * S:S] = f
            lens[s], labels[s], index[s] = len(f), list(lab), i
        out.append(dict(T=T, feat=feat, lens=lens, labels=labels, index=index))
    return out, skipped
