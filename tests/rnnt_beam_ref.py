"""The yardstick of the transducer beam search (include/klstm_rnnt.h states the search and its scores): the same search in plain torch on
the CPU, alpha column by column from the definition, run in float64 (the truth) and in float32 (the twin that sets the score's bar);
and the brute-force ranking of all label sequences by the lattice of tests/rnnt_ref.py."""
import itertools

import numpy as np
import torch

from tests.rnnt_ref import transducer

FINISHED, TRUNCATED, REJECTED, IDLE, PRUNED = 1, 2, 4, 8, 16
INF = float("inf")


def beam(enc, pred_fn, W, b, lens, blank, bos, B, N, max_len, dtype):
    """enc [T*S, J] (row t*S + s), W [V, J], b [V]: numpy; pred_fn(s, [bos, y_1 .. y_u]) -> the predictor's float32 row [J].  Returns per
    stream a dict: nbest [(tokens, score)], flags, steps (per step the (parent slot, label) of every new slot) and gap: the smallest
    margin of a comparison that decides the outcome (B-th against (B+1)-th candidate and the neighbours among the chosen, candidate
    against thr, an offered score against its neighbours in the list)."""
    S, J = len(lens), enc.shape[1]
    e3, Wt, bt = (torch.tensor(np.asarray(x), dtype=dtype) for x in (enc, W, b))
    e3 = e3.view(-1, S, J)
    out = []
    for s in range(S):
        Ts = int(lens[s])
        r = dict(nbest=[], steps=[], gap=INF, flags=IDLE if Ts == 0 else REJECTED if Ts < 0 or Ts > e3.shape[0] else 0)
        first = torch.full((max(Ts, 1),), -INF, dtype=dtype)
        first[0] = 0.0
        live = [((), first[:Ts])] if r["flags"] == 0 else []                  # (tokens, entry column)
        u = 0
        while live:
            cands = []
            for slot, (y, e) in enumerate(live):
                row = torch.tensor(pred_fn(s, [bos] + list(y)), dtype=dtype)
                lp = torch.log_softmax(torch.tanh(e3[:Ts, s] + row) @ Wt.T + bt, -1)
                alpha = [e[0]]
                for t in range(1, Ts):
                    alpha.append(torch.logaddexp(alpha[-1] + lp[t - 1, blank], e[t]))
                alpha = torch.stack(alpha)
                score = float(alpha[-1] + lp[-1, blank])
                r["gap"] = min([r["gap"]] + [abs(score - q[1]) for q in r["nbest"]])
                at = sum(q[1] >= score for q in r["nbest"])                  # a tie keeps the earlier entry
                r["nbest"] = (r["nbest"][:at] + [(list(y), score)] + r["nbest"][at:])[:N]
                entry = alpha[:, None] + lp
                prefix = torch.logsumexp(entry, 0)
                cands += [(float(prefix[k]), slot, k, entry[:, k]) for k in range(lp.shape[1]) if k != blank]
            thr = r["nbest"][N - 1][1] if len(r["nbest"]) == N else -INF
            r["gap"] = min([r["gap"]] + [abs(c[0] - thr) for c in cands])
            cands = sorted((c for c in cands if c[0] > thr), key=lambda c: (-c[0], c[1], c[2]))
            r["gap"] = min([r["gap"]] + [cands[i][0] - cands[i + 1][0] for i in range(min(B, len(cands) - 1))])
            if len(cands) > B:
                r["flags"] |= PRUNED
            if not cands:
                r["flags"] |= FINISHED
            elif u + 1 > max_len:
                r["flags"] |= TRUNCATED
                cands = []
            r["steps"].append([(c[1], c[2]) for c in cands[:B]])
            live = [(live[c[1]][0] + (c[2],), c[3]) for c in cands[:B]]
            u += 1
        out.append(r)
    return out


def brute_force(enc, pred_fn, W, b, blank, bos, max_len, N):
    """one stream: the N best of ALL label sequences up to max_len by the float64 full-sum log-probability of tests/rnnt_ref.py, and the
    smallest gap between neighbours among the N + 1 best"""
    V, scored = W.shape[0], []
    for n in range(max_len + 1):
        for y in itertools.product([k for k in range(V) if k != blank], repeat=n):
            pred = np.stack([pred_fn(0, [bos] + list(y[:i])) for i in range(n + 1)])
            scored.append((-float(transducer(enc, pred, W, b, [len(enc)], [list(y)], blank, torch.float64)["loss"][0]), list(y)))
    scored.sort(key=lambda q: -q[0])
    gap = min([INF] + [scored[i][0] - scored[i + 1][0] for i in range(min(N, len(scored) - 1))])
    return [(y, sc) for sc, y in scored[:N]], gap
