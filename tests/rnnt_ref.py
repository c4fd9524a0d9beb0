"""The yardstick of include/klstm_rnnt.h (which states the definition): one plain torch function on the CPU, run in float64 (the truth)
and in float32 (the twin that sets the bar of tests/test_rnnt_gpu.py).  Full logits, log_softmax, the alpha recursion as a Python loop
over the anti-diagonals, autograd for the gradients."""
import numpy as np
import torch

NEG = -1e30


def transducer(enc, pred, W, b, lens, labels, blank, dtype):
    """enc [T*S, J] (row t*S + s), pred [(Umax+1)*S, J] (row u*S + s), W [V, J], b [V]: numpy; lens, labels: S lengths and S label lists.
    Returns numpy arrays: loss [S] (0 for an idle stream), d_enc, d_pred, W_grad, b_grad of sum_s loss_s."""
    S, J = len(lens), enc.shape[1]
    leaf = [torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True) for x in (enc, pred, W, b)]
    e3, p3, Wt, bt = leaf[0].view(-1, S, J), leaf[1].view(-1, S, J), leaf[2], leaf[3]
    losses = []
    for s in range(S):
        Ts, y = int(lens[s]), [int(v) for v in labels[s]]
        U = len(y)
        if Ts == 0:
            losses.append(torch.zeros((), dtype=dtype))
            continue
        lp = torch.log_softmax(torch.tanh(e3[:Ts, s, None, :] + p3[None, :U + 1, s, :]) @ Wt.T + bt, -1)      # [Ts, U+1, V]
        lpb = lp[:, :, blank]
        lpy = lp[:, :U, :].gather(2, torch.tensor(y, dtype=torch.long).view(1, U, 1).expand(Ts, U, 1))[:, :, 0]    # [Ts, U]
        alpha = torch.full((U + 1,), NEG, dtype=dtype).index_put((torch.tensor([0]),), torch.zeros(1, dtype=dtype))
        for d in range(1, Ts + U):
            us = torch.arange(max(0, d - Ts + 1), min(U, d) + 1)
            ts = d - us
            stay = torch.where(ts >= 1, alpha[us] + lpb[(ts - 1).clamp(min=0), us], torch.full((), NEG, dtype=dtype))
            if U > 0:
                um = (us - 1).clamp(min=0)
                move = torch.where(us >= 1, alpha[um] + lpy[ts, um], torch.full((), NEG, dtype=dtype))
                stay = torch.logaddexp(stay, move)
            alpha = torch.full((U + 1,), NEG, dtype=dtype).index_put((us,), stay)
        losses.append(-(alpha[U] + lpb[Ts - 1, U]))
    loss = torch.stack(losses)
    loss.sum().backward()
    grads = [np.zeros(x.shape) if x.grad is None else x.grad.numpy() for x in leaf]
    return dict(loss=loss.detach().numpy(), d_enc=grads[0], d_pred=grads[1], W_grad=grads[2], b_grad=grads[3])


def rel_err(got, truth):
    """the project's measure: max|got - truth| / max|truth|"""
    truth = np.asarray(truth, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - truth).max() / max(np.abs(truth).max(), 1e-300))
