"""What the CTC objective costs next to the layer it trains: device time of klstm_ctc_eval (both chains + the combination) at
S = 8 / 16 / 32 streams, T = 500 / 1000 frames, L = 50 / 150 labels, K = 64 / 4096 classes, next to one bidirectional LSTMP layer's
forward + BPTT at 40/800/512 with the same S and T (in whatever mode the engines pick at that S).  The number to read is the loss as a
share of the layer's time.  Device events around warmed-up repeats that end in a synchronise, both legs in the same process.  Prints
one JSON line per shape and a table at the end (DESIGN.md 4h records it; profiles/ctc_probe.txt).

    python tools/ctc_probe.py [--iters 10] [--warmup 3] [--ctc-only]

--ctc-only: no layer leg (a rocprofv3 --kernel-trace --stats run of the loss alone)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kaldi_lstm_amd as k  # noqa: E402
from tests import regimes as rg  # noqa: E402

I, C, R = 40, 800, 512


def timed(step, iters, warmup):
    """device microseconds per call: events around `iters` calls, after `warmup`, ending in a synchronise"""
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def lengths(S, T, L):
    lens = [T - (37 * s) % (T // 4) for s in range(S)]
    return lens, [max(1, L - (5 * s) % (L // 2)) for s in range(S)]


def ctc_leg(S, T, L, K, iters, warmup):
    g = torch.Generator(device="cuda").manual_seed(S * 7 + T + L + K)
    lens, labs = lengths(S, T, L)
    labs[0] = L
    y = torch.softmax(torch.randn(T * S, K, generator=g, device="cuda") * 4.0, -1)
    labels = [(torch.randint(1, K, (n,), generator=g, device="cuda")).tolist() for n in labs]
    packed = k.ctc.pack_labels(labels, y.device)
    ld = torch.tensor(lens, dtype=torch.int32, device="cuda")
    diff = torch.empty_like(y)
    us = timed(lambda: k.ctc_eval(y, ld, packed, 0, diff), iters, warmup)
    loss, _ = k.ctc_eval(y, ld, packed, 0, diff)
    assert bool(torch.isfinite(loss).all())
    return us


def layer_leg(S, T, iters, warmup):
    lens, _ = lengths(S, T, 50)
    rng = np.random.RandomState(S + T)
    x = torch.from_numpy(rng.randn(T * S, I).astype(np.float32)).cuda()
    od = torch.from_numpy(rng.randn(T * S, 2 * R).astype(np.float32) * 1e-2).cuda()
    ld = torch.tensor(lens, dtype=torch.int32, device="cuda")
    bl = k.BidirectionalLstm(I, C, R, S)
    bl.set_params(rg.trained_params(I, C, R, 1), rg.trained_params(I, C, R, 2))
    out = torch.empty(T * S, 2 * R, device="cuda")
    ind = torch.empty(T * S, I, device="cuda")

    def step():
        bl.propagate(x, ld, out)
        bl.backpropagate(x, od, in_diff=ind, momentum=0.9)

    us = timed(step, iters, warmup)
    giveups = sum(e.profile_query("persist_giveups")[1] for e in (bl.fwd, bl.bwd))
    bl.close()
    return us, giveups


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ctc-only", action="store_true")
    a = ap.parse_args()
    rows = []
    for S in (8, 16, 32):
        for T in (500, 1000):
            layer, giveups = (None, 0) if a.ctc_only else layer_leg(S, T, max(2, a.iters // 2), max(1, a.warmup // 2))
            for K in (64, 4096):
                for L in (50, 150):
                    c = ctc_leg(S, T, L, K, a.iters, a.warmup)
                    r = {"S": S, "T": T, "L": L, "K": K, "ctc_us": round(c, 1),
                         "blstm_40_800_512_fwd_bptt_us": None if layer is None else round(layer, 1),
                         "ctc_share_of_layer_pct": None if layer is None else round(100.0 * c / layer, 2),
                         "persist_giveups": giveups}
                    rows.append(r)
                    print(json.dumps(r), flush=True)
    print("\n  S     T    L     K    ctc us    layer us   share")
    for r in rows:
        lay = r["blstm_40_800_512_fwd_bptt_us"]
        print(f"{r['S']:3d} {r['T']:5d} {r['L']:4d} {r['K']:5d} {r['ctc_us']:9.1f} " +
              (f"{lay:11.1f} {r['ctc_share_of_layer_pct']:6.2f}%" if lay is not None else "          -       -"))


if __name__ == "__main__":
    main()
