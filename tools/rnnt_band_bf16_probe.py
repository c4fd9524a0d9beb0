"""What the bf16 joint saves: device time of rnnt_band_eval with precision "f32" (krnnt_band_eval) and "bf16" (krnnt_band_eval_bf16) in
the same run, on the grid of tools/rnnt_band_probe.py: S = 8, T = 500, U = 50, J = 512, V in {64, 1024}, R in {4, 8, 16}, forward-only and
with gradients, bands from krnnt_band_from_frames on uniformly spread label frames.  Device events around warmed-up calls that end in a
synchronise, the legs alternating, TRIALS times; the median and the spread (min, max) are kept, and per pair whether the bf16 entry is
faster by more than the spread of either leg.  Writes profiles/rnnt_band_bf16_probe.json.

    python tools/rnnt_band_bf16_probe.py [--iters 5] [--warmup 2] [--out profiles/rnnt_band_bf16_probe.json]"""
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
from tools.rnnt_band_probe import J, S, T, TRIALS, U, WIDTHS, inputs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnnt_band_bf16_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    res = {"S": S, "T": T, "U": U, "J": J, "shapes": {}}
    for V in (64, 1024):
        enc, pred, W, b, lens, labels, packed, frames, out = inputs(T, U, V)
        legs, shape = {}, {}
        for R in WIDTHS:
            band = k.rnnt_band_from_frames([T] * S, labels, R, frames=frames)
            assert int(band.min()) >= 0, "the band must be feasible"
            for prec in ("f32", "bf16"):
                legs["forward_R%d_%s" % (R, prec)] = lambda band=band, R=R, prec=prec: k.rnnt_band_eval(
                    enc, pred, W, b, lens, packed, band, R, want_grads=False, precision=prec)
                legs["with_gradients_R%d_%s" % (R, prec)] = lambda band=band, R=R, prec=prec: k.rnnt_band_eval(
                    enc, pred, W, b, lens, packed, band, R, out=out, precision=prec)
            l32, l16 = [legs["forward_R%d_%s" % (R, prec)]()["loss"] for prec in ("f32", "bf16")]
            shape["R%d" % R] = {"workspace_bytes_f32": k.rnnt_band_workspace_bytes(T, S, U, R, J, V),
                                "workspace_bytes_bf16": k.rnnt_band_workspace_bytes(T, S, U, R, J, V, precision="bf16"),
                                "mean_loss_bf16_minus_f32": round(float((l16 - l32).mean()), 4)}
        times = {name: [] for name in legs}
        for _ in range(TRIALS):
            for name, leg in legs.items():
                times[name].append(timed(leg, a.iters, a.warmup))
        for name, v in times.items():
            print("V %-5d %-28s %10.1f us  (%.1f .. %.1f)" % (V, name, statistics.median(v), min(v), max(v)), flush=True)
        for R in WIDTHS:
            for kind in ("forward", "with_gradients"):
                t32, t16 = times["%s_R%d_f32" % (kind, R)], times["%s_R%d_bf16" % (kind, R)]
                m32, m16 = statistics.median(t32), statistics.median(t16)
                shape["R%d" % R][kind] = {"f32_us": round(m32, 1), "f32_us_min_max": [round(min(t32), 1), round(max(t32), 1)],
                                          "bf16_us": round(m16, 1), "bf16_us_min_max": [round(min(t16), 1), round(max(t16), 1)],
                                          "f32_over_bf16": round(m32 / m16, 2),
                                          "faster_by_more_than_the_spread": bool(m32 - m16 > max(max(t32) - min(t32), max(t16) - min(t16)))}
        res["shapes"]["V%d" % V] = shape
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"what": "device microseconds per call through rnnt_band_eval, median of %d trials of %d calls, both precisions in one run"
                           % (TRIALS, a.iters), "result": res}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
