"""The cost of the bidirectional wrapper: one BidirectionalLstm minibatch (propagate + backpropagate with KLSTM_BPTT_FUSE_UPDATE + update)
against the same work on two plain Engines -- the forward one on x, the backward one on a reversal of x built beforehand -- both with
"persist_verify" on, as the layer runs them.  40/800/512, T = 300, S = 4 and 8, ragged lengths.  Median wall time per minibatch over
--iters minibatches after --warmup.  Prints one JSON line per stream count (DESIGN.md 4f records the table).

    python tools/blstm_probe.py [--iters 50] [--warmup 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kaldi_lstm_amd as k  # noqa: E402
from tests import regimes as rg  # noqa: E402

I, C, R, T = 40, 800, 512, 300


def timed(step, iters, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    for S in (4, 8):
        lens = [T, T - 13, 257, 180, T - 1, 0, 271, T - 30][:S]
        rng = np.random.RandomState(S)
        pf, pb = rg.trained_params(I, C, R, 1), rg.trained_params(I, C, R, 2)
        x = torch.from_numpy((rng.randn(T * S, I)).astype(np.float32)).cuda()
        od = torch.from_numpy((rng.randn(T * S, 2 * R)).astype(np.float32)).cuda()
        ld = torch.tensor(lens, dtype=torch.int32, device="cuda")
        bl = k.BidirectionalLstm(I, C, R, S)
        bl.set_params(pf, pb)
        out = torch.empty(T * S, 2 * R, device="cuda")
        ind = torch.empty(T * S, I, device="cuda")

        def blstm():
            bl.propagate(x, ld, out)
            bl.backpropagate(x, od, in_diff=ind, momentum=0.9, flags=k.binding.BPTT_FUSE_UPDATE)
            bl.update(1e-6)

        ef, eb = k.Engine(I, C, R, S), k.Engine(I, C, R, S)
        for e, p in ((ef, pf), (eb, pb)):
            e.set_params(p)
            e.set_option("persist_verify", 1)
        xr = torch.empty_like(x)
        k.reverse_streams(x, ld, T, xr, k.REVERSE_SET)
        odf, odb = od[:, :R].contiguous(), od[:, R:].contiguous()
        of, ob = torch.empty(T * S, R, device="cuda"), torch.empty(T * S, R, device="cuda")
        idf, idb = torch.empty(T * S, I, device="cuda"), torch.empty(T * S, I, device="cuda")

        def two_engines():
            for e, xx, oo, dd, ii in ((ef, x, of, odf, idf), (eb, xr, ob, odb, idb)):
                e.reset([1] * S)
                e.propagate(xx, oo)
                e.backpropagate(xx, dd, ii, momentum=0.9, flags=k.binding.BPTT_FUSE_UPDATE)
                e.update(1e-6)

        t_two = timed(two_engines, a.iters, a.warmup)
        t_bl = timed(blstm, a.iters, a.warmup)
        t_two2 = timed(two_engines, a.iters, a.warmup)          # again: the order of the two runs should not matter
        giveups = sum(e.profile_query("persist_giveups")[1] for e in (bl.fwd, bl.bwd, ef, eb))
        base = min(t_two, t_two2)
        print(json.dumps({"shape": f"{I}/{C}/{R}", "S": S, "T": T, "two_engines_us": round(base, 1),
                          "two_engines_us_runs": [round(t_two, 1), round(t_two2, 1)], "blstm_us": round(t_bl, 1),
                          "overhead_pct": round(100.0 * (t_bl - base) / base, 2), "persist_giveups": giveups}), flush=True)
        for e in (bl, ef, eb):
            e.close()


if __name__ == "__main__":
    main()
