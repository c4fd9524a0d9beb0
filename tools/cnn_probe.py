"""What the CLDNN front end costs: device time of the four convolution entries and the two pooling entries of include/klstm_cnn.h at
whole-utterance size -- rows = 48000 (1500 frames x 32 streams), 11 x 40 inputs, patches of 8 every 1 (P = 33, K = 88), F = 128, pools
3 / 3 -- next to two yardsticks that are not the code under test: klstm_affine_propagate / _backpropagate / _gradient on an explicit
im2col matrix [rows P, K] built with torch.Tensor.unfold (what the library could do before: the matrix itself is not timed), and a plain
device copy of the convolution output's bytes, the floor of its write.  Device events around warmed-up repeats that end in a
synchronise, the legs alternating, TRIALS times; the median and the spread are kept.  Writes profiles/cnn_probe.json.

    python tools/cnn_probe.py [--rows 48000] [--iters 10] [--warmup 2] [--out profiles/cnn_probe.json]"""
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
N, ST, PD, PS, F, Z, G = 11, 40, 8, 1, 128, 3, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=48000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cnn_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    rows, P, K, geom = a.rows, 1 + (ST - PD) // PS, N * PD, (PD, PS, ST)
    Q = 1 + (P - Z) // G
    x = torch.randn(rows, N * ST, device="cuda")
    W = (torch.rand(F, K, device="cuda") - 0.5) * 0.6
    b = torch.zeros(F, device="cuda")
    out, od = torch.empty(rows, P * F, device="cuda"), torch.randn(rows, P * F, device="cuda")
    ind = torch.empty_like(x)
    fg, bg = torch.empty_like(W), torch.empty_like(b)
    Wc, bc = torch.zeros_like(W), torch.zeros_like(b)
    ws = torch.empty(k.conv_workspace_floats(rows, N * ST, P * F, PD, PS, ST), device="cuda")
    pooled, pd_ = torch.empty(rows, Q * F, device="cuda"), torch.randn(rows, Q * F, device="cuda")
    pin = torch.empty_like(out)
    # the explicit im2col matrix: [rows, n, P, pd] -> [rows P, n pd]
    col = x.view(rows, N, ST).unfold(2, PD, PS).permute(0, 2, 1, 3).reshape(rows * P, K).contiguous()
    out2, od2, col_diff = out.view(rows * P, F), od.view(rows * P, F), torch.empty_like(col)
    k.conv_propagate(x, W, b, out, geom)
    torch.cuda.synchronize()
    legs = {"copy_of_the_output": lambda: pin.copy_(out),
            "conv_propagate": lambda: k.conv_propagate(x, W, b, out, geom),
            "conv_backpropagate": lambda: k.conv_backpropagate(od, W, ind, geom),
            "conv_gradient": lambda: k.conv_gradient(x, od, fg, bg, geom, ws),
            "conv_update": lambda: k.conv_update(x, od, W, b, Wc, bc, 0.0, 0.0, 0.0, geom, ws),
            "pool_propagate": lambda: k.pool_propagate(out, pooled, (Z, G, F)),
            "pool_backpropagate": lambda: k.pool_backpropagate(out, pooled, pd_, pin, (Z, G, F))}
    base = {"affine_propagate_on_im2col": lambda: k.affine_propagate(col, W, b, out2),
            "affine_backpropagate_on_im2col": lambda: k.affine_backpropagate(od2, W, col_diff),
            "affine_gradient_on_im2col": lambda: k.affine_gradient(col, od2, fg, bg)}
    times = {name: [] for name in list(legs) + list(base)}
    for group in (legs, base):                           # the entries and the copy first, the im2col baselines after them
        for _ in range(TRIALS):
            for name, leg in group.items():
                times[name].append(timed(leg, a.iters, a.warmup))
    res = {"rows": rows, "geometry": [N, ST, PD, PS], "filters": F, "pool": [Z, G], "flop_per_product": 2 * rows * P * K * F,
           "input_bytes": x.numel() * 4, "output_bytes": out.numel() * 4, "im2col_bytes": col.numel() * 4, "legs": {}}
    for name, v in times.items():
        us = statistics.median(v)
        res["legs"][name] = {"us": round(us, 1), "us_min_max": [round(min(v), 1), round(max(v), 1)]}
        print("%-32s %10.1f us  (%.1f .. %.1f)" % (name, us, min(v), max(v)), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"what": "device microseconds per call through the Python entries, median of %d trials of %d calls" % (TRIALS, a.iters), "result": res}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
