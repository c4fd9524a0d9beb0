"""The yardstick of the greedy transducer decoder (include/klstm_rnnt.h states the loop): the plain frame-synchronous search in torch
on the CPU, one joint row per step, run in float64 (the truth) and in float32 (the twin that sets the score's bar)."""
import numpy as np
import torch

FINISHED, TRUNCATED, REJECTED, IDLE = 1, 2, 4, 8


def history_rows(table):
    """pred_fn(s, history) of the kernel tests: p_u = table[x_u] + 0.5 p_{u-1} over the history bos, y_1 .. y_u, in float64, rounded once"""
    def pred_fn(s, history):
        p = np.zeros(table.shape[1])
        for x in history:
            p = table[x] + 0.5 * p
        return p.astype(np.float32)
    return pred_fn


def greedy(enc, pred_fn, W, b, lens, blank, bos, max_symbols, max_len, dtype):
    """enc [T*S, J] (row t*S + s), W [V, J], b [V]: numpy; pred_fn(s, [bos, y_1 .. y_u]) -> the predictor's float32 row [J].  Returns per
    stream a dict: tokens, frames, score, flags, and gap: the smallest difference between the best and the second-best logit over the
    nodes of the path (inf when it has none)."""
    S, J = len(lens), enc.shape[1]
    e3, Wt, bt = (torch.tensor(np.asarray(x), dtype=dtype) for x in (enc, W, b))
    e3 = e3.view(-1, S, J)
    out = []
    for s in range(S):
        Ts = int(lens[s])
        r = dict(tokens=[], frames=[], score=torch.zeros((), dtype=dtype), gap=float("inf"),
                 flags=IDLE if Ts == 0 else REJECTED if Ts < 0 or Ts > e3.shape[0] else FINISHED)
        history, t, n = [bos], 0, 0
        while r["flags"] == FINISHED and t < Ts:
            a = torch.tanh(e3[t, s] + torch.tensor(pred_fn(s, history), dtype=dtype)) @ Wt.T + bt
            k = int((a == a.max()).nonzero()[0])          # a tie goes to the lower class
            top = torch.topk(a, 2).values
            r["gap"] = min(r["gap"], float(top[0] - top[1]))
            r["score"] = r["score"] + torch.log_softmax(a, -1)[k]
            if k == blank:
                t, n = t + 1, 0
                continue
            r["tokens"].append(k), r["frames"].append(t), history.append(k)
            n += 1
            if len(r["tokens"]) == max_len:
                r["flags"] = TRUNCATED
            elif n == max_symbols:
                t, n = t + 1, 0
        r["score"] = float(r["score"])
        out.append(r)
    return out
