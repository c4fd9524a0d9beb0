"""What forward-connection dropout costs: device time of kdrop_apply (include/klstm_dropout.h) forward in both modes, next to
klstm_time_shift with shift 0 on the same block -- the project's existing copy, and the yardstick: the time of the code under test is
never its own bar.  Shapes: a whole utterance batch of 1500 frames x 32 streams at 512 and at 1024 columns, and the trainer's
minibatch of 80 rows x 512.  Rows are pitched like a DeviceMatrix (a multiple of 64 floats), so the 16-byte path runs.  8 bytes of
traffic per element (4 in, 4 out) for all three legs.  Device events around warmed-up repeats that end in a synchronise, the legs
alternating, TRIALS times; the median and the spread are kept.  Writes profiles/dropout_probe.json (DESIGN.md 4v quotes it).

    python tools/dropout_probe.py [--iters 50] [--warmup 5] [--out profiles/dropout_probe.json]"""
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
SHAPES = [(1500, 32, 512), (1500, 32, 1024), (20, 4, 512)]       # (frames, streams, columns)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dropout_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    rows_out = []
    for T, S, cols in SHAPES:
        rows = T * S
        x = torch.randn(rows, cols, device="cuda")
        y = torch.empty_like(x)
        ids = torch.arange(S, dtype=torch.int32, device="cuda")
        legs = {"copy_time_shift_0": lambda: k.time_shift(x, y, 0),
                "dropout_element": lambda: k.dropout_apply(x, y, 0.8, 1234, 3, 1),
                "dropout_sequence": lambda: k.dropout_apply(x, y, 0.8, 1234, 0, 1, k.DROPOUT_SEQUENCE, S, ids)}
        times = {name: [] for name in legs}
        for _ in range(TRIALS):
            for name, leg in legs.items():
                times[name].append(timed(leg, a.iters, a.warmup))
        r = {"rows": rows, "streams": S, "cols": cols, "bytes": 8 * rows * cols}
        for name, v in times.items():
            us = statistics.median(v)
            r[name + "_us"] = round(us, 2)
            r[name + "_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
            r[name + "_GBps"] = round(r["bytes"] / us / 1e3, 1)
        for name in ("dropout_element", "dropout_sequence"):
            r[name + "_over_copy"] = round(r[name + "_us"] / r["copy_time_shift_0_us"], 3)
        rows_out.append(r)
        print("%6d x %4d  copy %8.2f us %7.1f GB/s | element %8.2f us %7.1f GB/s (%.2fx) | sequence %8.2f us %7.1f GB/s (%.2fx)" % (
            rows, cols, r["copy_time_shift_0_us"], r["copy_time_shift_0_GBps"], r["dropout_element_us"], r["dropout_element_GBps"],
            r["dropout_element_over_copy"], r["dropout_sequence_us"], r["dropout_sequence_GBps"], r["dropout_sequence_over_copy"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"what": "device microseconds per call through the Python entries, median of %d trials of %d calls; retention 0.8; 8 bytes "
                           "per element; the copy is klstm_time_shift with shift 0" % (TRIALS, a.iters), "rows": rows_out}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
