"""Yardsticks of the CTC tests (tests/test_ctc.py, tests/test_ctc_gpu.py), host only:
  oracle()         torch.nn.functional.ctc_loss on the CPU in float64 (or float32: "stock fp32", the bar's yardstick), the exact recipe
                   the kernel's semantics were fixed against
  brute_force()    -log of the sum over ALL alignments, float64, for tiny cases: pins the oracle independently of torch
  norm_twin()      the kernel's own recursion (normalised log domain, offsets summed in double) in numpy float32
  infeasible()     which streams klstm_ctc_eval must reject, from the lengths and labels alone
  make_case()      the seeded inputs of the parity cases: posteriors = fp32 softmax of scale * randn
  batch_twin()     the numpy twin of WholeUtteranceBatcher (include/klstm_trainer.hpp)"""
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
                    x1, x2 = pad[3:3 + N], np.where(np.concatenate([skip[2:], [False, False]]), pad[4:4 + N], NEG)
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
