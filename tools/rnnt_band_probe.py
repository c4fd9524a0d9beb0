"""What the band saves: device time and workspace bytes of krnnt_band_eval (include/klstm_rnnt.h, BAND-PRUNED TRAINING) forward-only and
with gradients at S = 8, T = 500, U = 50, J = 512, V in {64, 1024}, R in {4, 8, 16}, bands from krnnt_band_from_frames on uniformly spread
label frames, next to krnnt_eval on the same inputs (the yardstick, as it was).  Device events around warmed-up repeats that end in a
synchronise, the legs alternating, TRIALS times; the median and the spread are kept.  One shape that krnnt_eval refuses (S = 8, T = 3000,
U = 800, R = 8: T (U+1) S > 2^24) is run through the banded call once per trial as well.  Writes profiles/rnnt_band_probe.json
(DESIGN.md 4za).

    python tools/rnnt_band_probe.py [--iters 5] [--warmup 2] [--out profiles/rnnt_band_probe.json]"""
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
WIDTHS = (4, 8, 16)


def inputs(T, U, V):
    g = torch.Generator(device="cuda").manual_seed(V)
    enc, pred = torch.randn(T * S, J, device="cuda", generator=g), torch.randn((U + 1) * S, J, device="cuda", generator=g)
    W, b = (torch.rand(V, J, device="cuda", generator=g) - 0.5) * 0.6, torch.zeros(V, device="cuda")
    labels = [torch.randint(1, V, (U,), generator=torch.Generator().manual_seed(s)).tolist() for s in range(S)]
    frames = [[(2 * i + 1) * T // (2 * U) for i in range(U)] for _ in range(S)]           # uniformly spread label frames
    out = {"d_enc": torch.empty_like(enc), "d_pred": torch.empty_like(pred), "W_grad": torch.empty_like(W), "b_grad": torch.empty_like(b)}
    return enc, pred, W, b, torch.full((S,), T, dtype=torch.int32, device="cuda"), labels, k.ctc.pack_labels(labels, enc.device), frames, out


def summary(times, V):
    legs = {}
    for name, v in times.items():
        us = statistics.median(v)
        legs[name] = {"us": round(us, 1), "us_min_max": [round(min(v), 1), round(max(v), 1)]}
        print("V %-5d %-32s %10.1f us  (%.1f .. %.1f)" % (V, name, us, min(v), max(v)), flush=True)
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnnt_band_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    res = {"S": S, "T": T, "U": U, "J": J, "shapes": {}}
    for V in (64, 1024):
        enc, pred, W, b, lens, labels, packed, frames, out = inputs(T, U, V)
        legs = {"krnnt_eval_forward": lambda: k.rnnt_eval(enc, pred, W, b, lens, packed, want_grads=False),
                "krnnt_eval_with_gradients": lambda: k.rnnt_eval(enc, pred, W, b, lens, packed, out=out)}
        shape = {"krnnt_workspace_bytes": k.rnnt_workspace_bytes(T, S, U, J, V), "krnnt_forward_workspace_bytes": k.rnnt_workspace_bytes(T, S, U, J, V, False),
                 "band": {}}
        for R in WIDTHS:
            band = k.rnnt_band_from_frames([T] * S, labels, R, frames=frames)
            assert int(band.min()) >= 0, "the band must be feasible"
            legs["krnnt_band_eval_forward_R%d" % R] = lambda band=band, R=R: k.rnnt_band_eval(enc, pred, W, b, lens, packed, band, R, want_grads=False)
            legs["krnnt_band_eval_with_gradients_R%d" % R] = lambda band=band, R=R: k.rnnt_band_eval(enc, pred, W, b, lens, packed, band, R, out=out)
            full, banded = k.rnnt_eval(enc, pred, W, b, lens, packed, want_grads=False)["loss"], legs["krnnt_band_eval_forward_R%d" % R]()["loss"]
            shape["band"]["R%d" % R] = {"workspace_bytes": k.rnnt_band_workspace_bytes(T, S, U, R, J, V),
                                        "forward_workspace_bytes": k.rnnt_band_workspace_bytes(T, S, U, R, J, V, False),
                                        "mean_loss_banded_minus_full": round(float((banded - full).mean()), 4)}
        times = {name: [] for name in legs}
        for _ in range(TRIALS):
            for name, leg in legs.items():
                times[name].append(timed(leg, a.iters, a.warmup))
        shape["legs"] = summary(times, V)
        res["shapes"]["V%d" % V] = shape
    T2, U2, R2, V2 = 3000, 800, 8, 64                     # beyond krnnt_eval: T (U+1) S = 19.2 M nodes > 2^24
    enc, pred, W, b, lens, labels, packed, frames, out = inputs(T2, U2, V2)
    try:
        k.rnnt_workspace_bytes(T2, S, U2, J, V2)
        refused = False
    except k.KlstmError:
        refused = True
    band = k.rnnt_band_from_frames([T2] * S, labels, R2, frames=frames)
    times = {"krnnt_band_eval_with_gradients_R%d" % R2: [timed(lambda: k.rnnt_band_eval(enc, pred, W, b, lens, packed, band, R2, out=out), 2, 1)
                                                         for _ in range(3)]}
    loss = k.rnnt_band_eval(enc, pred, W, b, lens, packed, band, R2, want_grads=False)["loss"]
    res["beyond_the_full_path"] = {"S": S, "T": T2, "U": U2, "J": J, "V": V2, "R": R2, "krnnt_eval_refuses": refused,
                                   "workspace_bytes": k.rnnt_band_workspace_bytes(T2, S, U2, R2, J, V2),
                                   "losses_finite": bool(torch.isfinite(loss).all()) and int(band.min()) >= 0, "legs": summary(times, V2)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"what": "device microseconds per call through the Python entries, median of %d trials of %d calls" % (TRIALS, a.iters), "result": res}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
