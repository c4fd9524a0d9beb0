"""The yardstick of the simple-joiner loss and of the band rule (include/klstm_rnnt.h, THE SIMPLE JOINER and THE BAND RULE): plain torch on
the CPU at a given dtype (float64: the truth; float32: the twin that sets the bar).  The formula literally: the exp(x - max) product
form of the normaliser, the lattice in log space over the anti-diagonals, autograd of the loss for the gradients, occ from alpha and
beta."""
import numpy as np
import torch

from tests.rnnt_ref import NEG

FLT_MIN = float(np.finfo(np.float32).tiny)


def simple(am, lm, lens, labels, blank, dtype):
    """am [T*S, V] (row t*S + s), lm [(Umax+1)*S, V] (row u*S + s): numpy.  Returns numpy arrays: loss [S], d_am, d_lm of sum_s loss_s,
    occ [S, T, Umax+1]."""
    S, V = len(lens), am.shape[1]
    leaf = [torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True) for x in (am, lm)]
    a3, l3 = leaf[0].view(-1, S, V), leaf[1].view(-1, S, V)
    neg = torch.full((), NEG, dtype=dtype)
    occ = np.zeros((S, a3.shape[0], l3.shape[0]))
    losses = []
    for s in range(S):
        Ts, y = int(lens[s]), [int(v) for v in labels[s]]
        U = len(y)
        if Ts == 0:
            losses.append(torch.zeros((), dtype=dtype))
            continue
        a, l = a3[:Ts, s], l3[:U + 1, s]
        ma, ml = a.max(1, keepdim=True)[0].detach(), l.max(1, keepdim=True)[0].detach()
        P = (torch.exp(a - ma) @ torch.exp(l - ml).T).clamp_min(FLT_MIN)                                       # [Ts, U+1]
        lse = ma + ml.T + torch.log(P)
        lpb = a[:, None, blank] + l[None, :, blank] - lse
        yi = torch.tensor(y, dtype=torch.long)
        lpy = a[:, yi] + l[torch.arange(U), yi][None, :] - lse[:, :U]                                          # [Ts, U]
        rows = [torch.full((U + 1,), NEG, dtype=dtype).index_put((torch.tensor([0]),), torch.zeros(1, dtype=dtype))]
        for d in range(1, Ts + U):
            us = torch.arange(max(0, d - Ts + 1), min(U, d) + 1)
            ts = d - us
            stay = torch.where(ts >= 1, rows[-1][us] + lpb[(ts - 1).clamp(min=0), us], neg)
            if U > 0:
                um = (us - 1).clamp(min=0)
                stay = torch.logaddexp(stay, torch.where(us >= 1, rows[-1][um] + lpy[ts, um], neg))
            rows.append(torch.full((U + 1,), NEG, dtype=dtype).index_put((us,), stay))
        loss = -(rows[-1][U] + lpb[Ts - 1, U])
        losses.append(loss)
        with torch.no_grad():                            # occ = w_b + w_y from alpha (the rows) and beta
            ug = torch.arange(U + 1)
            alpha = torch.stack(rows)[torch.arange(Ts)[:, None] + ug[None, :], ug[None, :]]                    # alpha(t, u) = row t + u at u
            beta = torch.full((Ts + 1, U + 2), NEG, dtype=dtype)
            beta[Ts, U] = 0                              # beta(T, U) = 0: the last blank leaves the lattice
            lpy_pad = torch.cat([lpy, torch.full((Ts, 1), NEG, dtype=dtype)], 1)
            for d in range(Ts + U - 1, -1, -1):
                us = torch.arange(max(0, d - Ts + 1), min(U, d) + 1)
                ts = d - us
                beta[ts, us] = torch.logaddexp(beta[ts + 1, us] + lpb[ts, us], beta[ts, us + 1] + lpy_pad[ts, us]).clamp_min(NEG)
            wb = torch.exp(alpha + lpb + beta[1:, :U + 1] + loss)
            wy = torch.exp(alpha[:, :U] + lpy + beta[:Ts, 1:U + 1] + loss)
            occ[s, :Ts, :U + 1] = wb.numpy()
            occ[s, :Ts, :U] += wy.numpy()
    loss = torch.stack(losses)
    loss.sum().backward()
    grads = [np.zeros(x.shape) if x.grad is None else x.grad.numpy() for x in leaf]
    return dict(loss=loss.detach().numpy(), d_am=grads[0], d_lm=grads[1], occ=occ)


def band_rule(occ, Ts, U, R):
    """THE BAND RULE for one stream, transcribed; occ [T, Umax+1] float32.  [] for an idle stream."""
    if Ts <= 0:
        return []
    hi = max(0, U + 1 - R)
    w = np.zeros((Ts, hi + 1))                           # w(t, k), every k at once: float64, the terms added in the order of r
    for r in range(min(R, U + 1)):
        n = min(hi, U - r) + 1                           # the k with k + r <= U
        w[:, :n] += occ[:Ts, r:r + n].astype(np.float64)
    c = [int(k) for k in np.argmax(w, axis=1)]           # the first of equal maxima: the lower k
    c[0] = 0
    c[-1] = hi
    u0 = list(np.maximum.accumulate(c))
    for t in range(Ts - 2, -1, -1):
        u0[t] = max(u0[t], u0[t + 1] - (R - 1))
    return [int(v) for v in u0] if u0[0] == 0 else [-1] * Ts
