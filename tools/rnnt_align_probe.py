"""What a transducer forced alignment costs next to the forward-only loss of the same shape: device time of rnnt_align (full lattice;
banded at R = 8 with the f32 and with the bf16 joint) and, in the same run and alternating with them, of rnnt_eval / rnnt_band_eval with
want_grads=False, at S = 8, T = 500, U = 50, J = 512, V in {64, 1024} (the inputs of tools/rnnt_band_probe.py).  An align call runs the
same joint kernel, one lattice direction in place of two and no weights kernel, but ends in a serial backtrace; the legs with U = 0
(T diagonals of one node and T backtrace steps behind a joint of T nodes) bound what recursion and backtrace cost by themselves.
Device events around warmed-up calls that end in a synchronise, TRIALS times; the median and the spread (min, max) are kept.  Writes
profiles/rnnt_align_probe.json.

    python tools/rnnt_align_probe.py [--iters 5] [--warmup 2] [--out profiles/rnnt_align_probe.json]"""
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
from tools.rnnt_band_probe import J, S, T, TRIALS, U, inputs, summary  # noqa: E402

R = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnnt_align_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    res = {"S": S, "T": T, "U": U, "J": J, "R": R, "shapes": {}}
    for V in (64, 1024):
        enc, pred, W, b, lens, labels, packed, frames, _ = inputs(T, U, V)
        band = k.rnnt_band_from_frames([T] * S, labels, R, frames=frames)
        none, band0 = k.ctc.pack_labels([[]] * S, enc.device), torch.zeros(S, T, dtype=torch.int32, device="cuda")
        legs = {"eval_full_forward": lambda: k.rnnt_eval(enc, pred, W, b, lens, packed, want_grads=False),
                "align_full": lambda: k.rnnt_align(enc, pred, W, b, lens, packed),
                "align_full_U0": lambda: k.rnnt_align(enc, pred[:S], W, b, lens, none),
                "align_band_U0": lambda: k.rnnt_align(enc, pred[:S], W, b, lens, none, band_lo=band0, R=R)}
        for prec in ("f32", "bf16"):
            legs["eval_band_forward_" + prec] = lambda prec=prec: k.rnnt_band_eval(enc, pred, W, b, lens, packed, band, R, want_grads=False, precision=prec)
            legs["align_band_" + prec] = lambda prec=prec: k.rnnt_align(enc, pred, W, b, lens, packed, band_lo=band, R=R, precision=prec)
        full, inband = legs["align_full"](), legs["align_band_f32"]()
        own = k.rnnt_band_from_frames([T] * S, labels, R, frames=full["frames"])               # the band around the model's own alignment
        times = {name: [] for name in legs}
        for _ in range(TRIALS):
            for name, leg in legs.items():
                times[name].append(timed(leg, a.iters, a.warmup))
        shape = {"legs": summary(times, V), "workspace_bytes_full": k.rnnt_align_workspace_bytes(T, S, U),
                 "workspace_bytes_band": k.rnnt_align_workspace_bytes(T, S, U, J, V, R=R),
                 "mean_score_full": round(float(full["score"].mean()), 3), "mean_score_band": round(float(inband["score"].mean()), 3),
                 "own_band_feasible": bool(int(own.min()) >= 0)}
        for kind, ref in (("align_full", "eval_full_forward"), ("align_band_f32", "eval_band_forward_f32"), ("align_band_bf16", "eval_band_forward_bf16")):
            ta, te = times[kind], times[ref]
            shape[kind + "_over_forward"] = round(statistics.median(ta) / statistics.median(te), 3)
            shape[kind + "_slower_by_more_than_the_spread"] = bool(statistics.median(ta) - statistics.median(te) > max(max(ta) - min(ta), max(te) - min(te)))
        res["shapes"]["V%d" % V] = shape
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"what": "device microseconds per call, median of %d trials of %d calls, all legs in one run" % (TRIALS, a.iters), "result": res}, fh,
                  indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
