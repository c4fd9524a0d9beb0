"""The yardstick of transducer forced alignment (include/klstm_rnnt.h, FORCED ALIGNMENT): full logits and log_softmax in the given dtype
(float64: the truth, float32: the twin; bf16=True: the two roundings hb, Wb of THE BF16 JOINT), then the max-plus recursion of the
definition node by node with the `>` rule, an optional band, and the backtrace."""
import numpy as np
import torch

from tests.rnnt_band_bf16_ref import bf
from tests.rnnt_ref import NEG


def planes(enc, pred, W, b, lens, labels, blank, dtype, bf16=False):
    """per stream (lpb [T_s, U+1], lpy [T_s, U]) as numpy arrays of the dtype; None for an idle stream"""
    S, J = len(lens), enc.shape[1]
    e3, p3, Wt, bt = [torch.tensor(np.asarray(x), dtype=dtype) for x in (enc, pred, W, b)]
    e3, p3, out = e3.view(-1, S, J), p3.view(-1, S, J), []
    for s in range(S):
        Ts, y = int(lens[s]), [int(v) for v in labels[s]]
        if Ts == 0:
            out.append(None)
            continue
        h = torch.tanh(e3[:Ts, s, None, :] + p3[None, :len(y) + 1, s, :])
        lp = torch.log_softmax((bf(h) @ bf(Wt).T if bf16 else h @ Wt.T) + bt, -1)
        out.append((lp[:, :, blank].numpy(), lp[:, :len(y), :].gather(2, torch.tensor(y, dtype=torch.long).view(1, -1, 1).expand(Ts, -1, 1))[:, :, 0].numpy()))
    return out


inband = lambda band_row, R, t, u: band_row is None or band_row[t] <= u < band_row[t] + R


def viterbi(lpb, lpy, band_row=None, R=None):
    """one stream: (score, frames, logp, the smallest |x1 - x2| over the nodes of the best path); arithmetic in the planes' dtype"""
    Ts, U1 = lpb.shape
    dt, neg = lpb.dtype.type, lpb.dtype.type(NEG)
    v, take, gap = np.full((Ts, U1), neg, lpb.dtype), np.zeros((Ts, U1), bool), np.zeros((Ts, U1))
    for t in range(Ts):
        for u in range(U1):
            if not inband(band_row, R, t, u):
                continue
            if t == 0 and u == 0:
                v[0, 0] = dt(0)
                continue
            x1 = v[t - 1, u] + lpb[t - 1, u] if t > 0 else neg
            x2 = v[t, u - 1] + lpy[t, u - 1] if u > 0 else neg
            take[t, u] = x2 > x1 and x2 > -1e29
            v[t, u], gap[t, u] = max(x2 if take[t, u] else x1, neg), abs(float(x1) - float(x2))
    t, u, frames, logp, margin = Ts - 1, U1 - 1, [0] * (U1 - 1), [0.0] * (U1 - 1), np.inf
    while t > 0 or u > 0:
        margin = min(margin, gap[t, u])
        if take[t, u]:
            u -= 1
            frames[u], logp[u] = t, float(lpy[t, u])
        else:
            t -= 1
    return float(v[Ts - 1, U1 - 1] + lpb[Ts - 1, U1 - 1]), frames, logp, margin


def rescore(lpb, lpy, frames, band_row=None, R=None):
    """the log-probability of the path that enters label i at frames[i - 1], on the given planes; NEG if it leaves the band"""
    Ts, total, u = lpb.shape[0], 0.0, 0
    for t in range(Ts):
        while u < len(frames) and frames[u] == t:
            total, u = total + float(lpy[t, u]), u + 1
            if not inband(band_row, R, t, u):
                return NEG
        if not inband(band_row, R, t, u):
            return NEG
        total += float(lpb[t, u])
    return total if u == len(frames) else NEG


def align(enc, pred, W, b, lens, labels, blank, dtype, band=None, R=None, bf16=False):     # (viterbi() per stream, the planes)
    pl = planes(enc, pred, W, b, lens, labels, blank, dtype, bf16)
    return [None if p is None else viterbi(*p, None if band is None else band[s], R) for s, p in enumerate(pl)], pl
