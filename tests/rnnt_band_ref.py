"""The yardstick of band-pruned transducer training (include/klstm_rnnt.h, BAND-PRUNED TRAINING): tests/rnnt_ref.py's function with the
band applied.  Full logits, log_softmax, the alpha recursion over the anti-diagonals with every node outside the band set to NEG,
autograd for the gradients; run in float64 (the truth) and in float32 (the twin)."""
import numpy as np
import torch

from tests.rnnt_ref import NEG


def transducer(enc, pred, W, b, lens, labels, blank, band_lo, R, dtype):
    """The arguments of rnnt_ref.transducer plus band_lo (S rows, u0(t) for t < T_s) and the width R.  Returns the same dict."""
    S, J = len(lens), enc.shape[1]
    leaf = [torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True) for x in (enc, pred, W, b)]
    e3, p3, Wt, bt = leaf[0].view(-1, S, J), leaf[1].view(-1, S, J), leaf[2], leaf[3]
    neg = torch.full((), NEG, dtype=dtype)
    losses = []
    for s in range(S):
        Ts, y = int(lens[s]), [int(v) for v in labels[s]]
        U = len(y)
        if Ts == 0:
            losses.append(torch.zeros((), dtype=dtype))
            continue
        u0 = torch.tensor([int(v) for v in band_lo[s][:Ts]]).view(Ts, 1)
        ug = torch.arange(U + 1).view(1, U + 1)
        inband = (ug >= u0) & (ug < u0 + R)                                                                      # [Ts, U+1]
        lp = torch.log_softmax(torch.tanh(e3[:Ts, s, None, :] + p3[None, :U + 1, s, :]) @ Wt.T + bt, -1)
        lpb = lp[:, :, blank]
        lpy = lp[:, :U, :].gather(2, torch.tensor(y, dtype=torch.long).view(1, U, 1).expand(Ts, U, 1))[:, :, 0]
        alpha = torch.full((U + 1,), NEG, dtype=dtype).index_put((torch.tensor([0]),), torch.zeros(1, dtype=dtype))
        for d in range(1, Ts + U):
            us = torch.arange(max(0, d - Ts + 1), min(U, d) + 1)
            ts = d - us
            stay = torch.where(ts >= 1, alpha[us] + lpb[(ts - 1).clamp(min=0), us], neg)
            if U > 0:
                um = (us - 1).clamp(min=0)
                stay = torch.logaddexp(stay, torch.where(us >= 1, alpha[um] + lpy[ts, um], neg))
            alpha = torch.full((U + 1,), NEG, dtype=dtype).index_put((us,), torch.where(inband[ts, us], stay, neg))
        losses.append(-(alpha[U] + lpb[Ts - 1, U]))
    loss = torch.stack(losses)
    loss.sum().backward()
    grads = [np.zeros(x.shape) if x.grad is None else x.grad.numpy() for x in leaf]
    return dict(loss=loss.detach().numpy(), d_enc=grads[0], d_pred=grads[1], W_grad=grads[2], b_grad=grads[3])
