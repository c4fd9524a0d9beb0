"""The yardstick of the bf16 joint (include/klstm_rnnt.h, THE BF16 JOINT): tests/rnnt_band_ref.py's function with the three roundings of
the definition, each through .to(torch.bfloat16).  hb = bf(tanh(.)) and Wb = bf(W) enter the product; its backward rounds the incoming g,
multiplies with the rounded operands and hands d h on as if the rounding of h were the identity.  b stays outside the product, so
b_grad sums the unrounded g.  Evaluated in float64 it gives the quantisation error of the definition itself (products of bf16 values and
their sums are then exact to 2^-53)."""
import numpy as np
import torch

from tests.rnnt_ref import NEG


def bf(x):
    return x.to(torch.bfloat16).to(x.dtype)


class Bf16Joint(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, W):
        hb, Wb = bf(h), bf(W)
        ctx.save_for_backward(hb, Wb)
        return hb @ Wb.T

    @staticmethod
    def backward(ctx, g):
        hb, Wb = ctx.saved_tensors
        gb = bf(g)
        return gb @ Wb, gb.reshape(-1, gb.shape[-1]).T @ hb.reshape(-1, hb.shape[-1])


def transducer(enc, pred, W, b, lens, labels, blank, band_lo, R, dtype):
    """The arguments and the result of rnnt_band_ref.transducer; only the line of the logits differs from it."""
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
        inband = (ug >= u0) & (ug < u0 + R)
        lp = torch.log_softmax(Bf16Joint.apply(torch.tanh(e3[:Ts, s, None, :] + p3[None, :U + 1, s, :]), Wt) + bt, -1)
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
