"""What a fused label language model costs the CTC prefix beam search (klstm_ctc_beam_decode_lm; DESIGN.md 4l;
profiles/ctc_beam_lm_probe.txt): device time per frame of the search chain at T = 1000, K = 64 on the peaked posteriors of
tools/ctc_decode_probe.py (all streams of full length, so the time of the call is the time of one chain), without references, for
  none       ctc_beam_decode without an LM (the call as it was)
  bigram     Q = 65 states: 33 KB of tables
  trigram    Q = 4097 states: 2 MB of tables, next states spread over all of them
  qN         Q = N states (q129, q192, ...), next states spread like the trigram's: table sizes between the two, for the threshold
and beam / candidates 4/4, 16/8, 64/32.  Every figure is the MEDIAN over --repeats timings of --iters calls each (device events around
warmed-up calls that end in a synchronise), with the spread (max - min) / median of those timings next to it.  `plan` is where the
tables were read from (klstm_ctc_beam_lm_resident): lds or global.  To time the plan a shape does NOT take, load a build of the same
sources with another threshold (-DKLSTM_BEAM_LM_RESIDENT_BYTES=0: always global) through KLSTM_LIB_PATH.  One JSON line per shape and a
table at the end.

    python tools/ctc_beam_lm_probe.py [--iters 5] [--warmup 2] [--repeats 5] [--frames 1000] [--streams 1,8,32] [--classes 64]
                                      [--configs 4/4,16/8,64/32] [--setups none,bigram,trigram]

--setups none runs on a build without the feature too (the comparison with the commit before it)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kaldi_lstm_amd as k  # noqa: E402
from tools.ctc_decode_probe import peaked, timed  # noqa: E402


def tables(kind, K, seed=0):
    """-> (next, weight, final): weights in [0.2, 1.2), a tenth of them 0"""
    rng = np.random.RandomState(seed)
    Q = K + 1 if kind == "bigram" else K * K + 1 if kind == "trigram" else int(kind[1:])
    q, c = np.meshgrid(np.arange(Q), np.arange(K), indexing="ij")
    nxt = (1 + c if kind == "bigram" else 1 + (q * 31 + c * K + c) % (Q - 1)).astype(np.int32)
    wt = (0.2 + rng.rand(Q, K)).astype(np.float32)
    wt[rng.rand(Q, K) < 0.1] = 0.0
    return nxt, wt, (0.5 + rng.rand(Q)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", default="1000")
    ap.add_argument("--streams", default="1,8,32")
    ap.add_argument("--classes", default="64")
    ap.add_argument("--configs", default="4/4,16/8,64/32")
    ap.add_argument("--setups", default="none,bigram,trigram")
    a = ap.parse_args()
    ints = lambda v: [int(x) for x in v.split(",")]   # noqa: E731
    configs = [tuple(int(x) for x in v.split("/")) for v in a.configs.split(",")]
    setups = a.setups.split(",")
    rows = []
    for K in ints(a.classes):
        lms = {s: k.CtcLabelLm(*tables(s, K)) for s in setups if s != "none"}
        for S in ints(a.streams):
            for T in ints(a.frames):
                if T * S > 65535:
                    continue
                g = torch.Generator(device="cuda").manual_seed(S * 7 + T + K)
                lens = [T] * S
                y, _ = peaked(T, S, K, lens, g)
                ld = torch.tensor(lens, dtype=torch.int32, device="cuda")
                for B, C in configs:
                    r = {"T": T, "S": S, "K": K, "beam": B, "cands": C}
                    for s in setups:
                        kw = {} if s == "none" else {"lm": lms[s]}
                        ts = [timed(lambda: k.ctc_beam_decode(y, ld, 0, B, C, min(B, 4), **kw), a.iters, a.warmup if i == 0 else 0)
                              for i in range(a.repeats)]
                        med = statistics.median(ts)
                        r[s + "_us_per_frame"] = round(med / T, 3)
                        r[s + "_spread"] = round((max(ts) - min(ts)) / med, 4)
                        if s != "none":
                            r[s + "_plan"] = "lds" if lms[s].resident(B, C) else "global"
                            r[s + "_states"] = lms[s].states
                    rows.append(r)
                    print(json.dumps(r), flush=True)
                del y
    print("\n    T   S   K  beam/cands " + "".join(f" {s + ' us/frame':>17s} {'spread':>7s} {'plan':>6s}" for s in setups))
    for r in rows:
        print(f"{r['T']:5d} {r['S']:3d} {r['K']:3d} {'%d/%d' % (r['beam'], r['cands']):>11s} " +
              "".join(f" {r[s + '_us_per_frame']:17.3f} {100 * r[s + '_spread']:6.1f}% {r.get(s + '_plan', '-'):>6s}" for s in setups))


if __name__ == "__main__":
    main()
