"""What transducer training costs: device time of krnnt_eval (include/klstm_rnnt.h) forward-only and with gradients at S = 8, T = 500,
U = 50, J = 512, V in {64, 1024}, next to the composition the library offered before on materialised [S T (U+1), J] rows: an elementwise
tanh(e + p) in torch, klstm_affine_propagate, and the log-softmax of klstm_log_softmax_scatter (forward only: there was no lattice
recursion to compare the rest with).  Device events around warmed-up repeats that end in a synchronise, the legs alternating, TRIALS
times; the median and the spread are kept, and the bytes each side allocates.  Writes profiles/rnnt_probe.json.

    python tools/rnnt_probe.py [--iters 5] [--warmup 2] [--out profiles/rnnt_probe.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import kaldi_lstm_amd as k  # noqa: E402
from tools.ctc_probe import timed  # noqa: E402

TRIALS = 5
S, T, U, J = 8, 500, 50, 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnnt_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    res = {"S": S, "T": T, "U": U, "J": J, "shapes": {}}
    for V in (64, 1024):
        g = torch.Generator(device="cuda").manual_seed(V)
        enc, pred = torch.randn(T * S, J, device="cuda", generator=g), torch.randn((U + 1) * S, J, device="cuda", generator=g)
        W, b = (torch.rand(V, J, device="cuda", generator=g) - 0.5) * 0.6, torch.zeros(V, device="cuda")
        labels = [torch.randint(1, V, (U,), generator=torch.Generator().manual_seed(s)).tolist() for s in range(S)]
        packed = k.ctc.pack_labels(labels, enc.device)
        lens = torch.full((S,), T, dtype=torch.int32, device="cuda")
        N = S * T * (U + 1)
        out = {"d_enc": torch.empty_like(enc), "d_pred": torch.empty_like(pred), "W_grad": torch.empty_like(W), "b_grad": torch.empty_like(b)}
        h, logits, logp = torch.empty(N, J, device="cuda"), torch.empty(N, V, device="cuda"), torch.empty(N, V, device="cuda")
        rows = torch.arange(N, dtype=torch.int32, device="cuda")
        e3, p3 = enc.view(T, 1, S, J), pred.view(1, U + 1, S, J)

        def composition():
            torch.tanh(torch.add(e3, p3, out=h.view(T, U + 1, S, J)), out=h.view(T, U + 1, S, J))
            k.affine_propagate(h, W, b, logits)
            k.log_softmax_scatter(logits, rows, logp, k.SCORE_LOGPOST)

        legs = {"krnnt_eval_forward": lambda: k.rnnt_eval(enc, pred, W, b, lens, packed, want_grads=False),
                "krnnt_eval_with_gradients": lambda: k.rnnt_eval(enc, pred, W, b, lens, packed, out=out),
                "composition_forward": composition}
        times = {name: [] for name in legs}
        for _ in range(TRIALS):
            for name, leg in legs.items():
                times[name].append(timed(leg, a.iters, a.warmup))
        shape = {"flop_per_product": 2 * N * J * V, "krnnt_workspace_bytes": k.rnnt_workspace_bytes(T, S, U, J, V),
                 "composition_bytes": 4 * (h.numel() + logits.numel() + logp.numel()), "legs": {}}
        for name, v in times.items():
            us = statistics.median(v)
            shape["legs"][name] = {"us": round(us, 1), "us_min_max": [round(min(v), 1), round(max(v), 1)]}
            print("V %-5d %-28s %10.1f us  (%.1f .. %.1f)" % (V, name, us, min(v), max(v)), flush=True)
        res["shapes"]["V%d" % V] = shape
        del h, logits, logp
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"what": "device microseconds per call through the Python entries, median of %d trials of %d calls" % (TRIALS, a.iters), "result": res}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
