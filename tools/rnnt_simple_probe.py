"""What the first pass of pruned transducer training costs: device time of krnnt_simple_eval (include/klstm_rnnt.h, THE SIMPLE JOINER)
forward-only and with gradients plus occ, and of krnnt_band_from_occupation on that occ at R = 8, at S = 8, T = 500, U = 50, V in
{64, 1024}, next to krnnt_eval with gradients (the full lattice it stands in for) and krnnt_band_eval with gradients at R = 8, J = 512
in the band just derived.  Device events around warmed-up repeats that end in a synchronise, the legs alternating, TRIALS times; the
median and the spread are kept.  Writes profiles/rnnt_simple_probe.json.

    python tools/rnnt_simple_probe.py [--iters 5] [--warmup 2] [--out profiles/rnnt_simple_probe.json]"""
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
S, T, U, J, R = 8, 500, 50, 512, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnnt_simple_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    res = {"S": S, "T": T, "U": U, "J": J, "R": R, "shapes": {}}
    for V in (64, 1024):
        g = torch.Generator(device="cuda").manual_seed(V)
        rnd = lambda *shape: torch.randn(*shape, device="cuda", generator=g)
        enc, pred, W, b = rnd(T * S, J), rnd((U + 1) * S, J), (torch.rand(V, J, device="cuda", generator=g) - 0.5) * 0.6, torch.zeros(V, device="cuda")
        am, lm = rnd(T * S, V), rnd((U + 1) * S, V)
        labels = [torch.randint(1, V, (U,), generator=torch.Generator().manual_seed(s)).tolist() for s in range(S)]
        am[:, 0] += 8                                      # a trained-looking am over the noise: blank everywhere but at the uniformly
        for s in range(S):                                 # spread label frames, so that the occupation follows an alignment
            for i, y in enumerate(labels[s]):
                row = ((2 * i + 1) * T // (2 * U)) * S + s
                am[row, 0] -= 8
                am[row, y] += 8
        lens, packed = torch.full((S,), T, dtype=torch.int32, device="cuda"), k.ctc.pack_labels(labels, enc.device)
        out = {"d_enc": torch.empty_like(enc), "d_pred": torch.empty_like(pred), "W_grad": torch.empty_like(W), "b_grad": torch.empty_like(b)}
        sout = {"d_am": torch.empty_like(am), "d_lm": torch.empty_like(lm), "occ": torch.empty(S, T, U + 1, device="cuda")}
        occ = k.rnnt_simple_eval(am, lm, lens, packed, want_occ=True, out=sout)["occ"]
        band = k.rnnt_band_from_occupation(occ, lens, packed, R)
        assert int(band.min()) >= 0, "the band must be feasible"
        legs = {"krnnt_simple_eval_forward": lambda: k.rnnt_simple_eval(am, lm, lens, packed, want_grads=False),
                "krnnt_simple_eval_with_gradients_and_occ": lambda: k.rnnt_simple_eval(am, lm, lens, packed, want_occ=True, out=sout),
                "krnnt_band_from_occupation_R%d" % R: lambda: k.rnnt_band_from_occupation(occ, lens, packed, R),
                "krnnt_eval_with_gradients": lambda: k.rnnt_eval(enc, pred, W, b, lens, packed, out=out),
                "krnnt_band_eval_with_gradients_R%d" % R: lambda: k.rnnt_band_eval(enc, pred, W, b, lens, packed, band, R, out=out)}
        times = {name: [] for name in legs}
        for _ in range(TRIALS):
            for name, leg in legs.items():
                times[name].append(timed(leg, a.iters, a.warmup))
        shape = {"krnnt_simple_workspace_bytes": k.rnnt_simple_workspace_bytes(T, S, U, V), "legs": {}}
        for name, v in times.items():
            us = statistics.median(v)
            shape["legs"][name] = {"us": round(us, 1), "us_min_max": [round(min(v), 1), round(max(v), 1)]}
            print("V %-5d %-44s %10.1f us  (%.1f .. %.1f)" % (V, name, us, min(v), max(v)), flush=True)
        res["shapes"]["V%d" % V] = shape
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"what": "device microseconds per call through the Python entries, median of %d trials of %d calls" % (TRIALS, a.iters), "result": res}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
