"""What CTC best-path decoding costs (klstm_ctc_decode; profiles/ctc_decode_probe.txt): device time of the whole call --
row argmax, collapse, path score, edit distance -- at (T, S, K) from {300, 1000, 2000} x {4, 8, 32} x {48, 1024, 16624} with ragged
lengths, next to its yardsticks on the same tensor in the same process, alternating with it:
  call           ctc_greedy_decode with references (both kernels, edit distance included)
  no_refs        the same without references: the argmax launch plus collapse and score only -- an UPPER bound of the argmax kernel's
                 time (the per-kernel split is in profiles/ctc_decode_rocprofv3_kernel_stats.txt, a run of its own)
  torch_argmax   torch.argmax(net_out, dim=1) alone: reads the same bytes (padding rows too), does none of the rest
  host           what a user had before: net_out.cpu(), numpy argmax, Python collapse (wall clock, once)
  read GB/s      bytes the call must read (valid rows x K x 4) over the no_refs time, next to `copy GB/s`: a plain device copy of that
                 many bytes (bytes copied over time: the copy also writes them)
  share          the call as a share of one bidirectional 40/800/512 layer's forward at that T and S
Device events around warmed-up repeats that end in a synchronise.  One JSON line per shape and a table at the end.

    python tools/ctc_decode_probe.py [--iters 10] [--warmup 3] [--call-only] [--frames 300,1000,2000] [--streams 4,8,32] [--classes 48,1024,16624]

--call-only: no yardsticks and no layer leg (a rocprofv3 --kernel-trace --stats run of the call alone; geometry comparisons)."""
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


def lengths(S, T):
    return [T - (37 * s) % (T // 4) for s in range(S)]


def peaked(T, S, K, lens, g):
    """posteriors whose best path looks like speech: runs of 3..8 frames of one class, a third of them blank; labels = the collapsed
    path with every tenth token changed, so the edit distance works on a hypothesis close to its reference"""
    run = torch.randint(0, K, (T // 3 + 2, S), generator=g, device="cuda")
    run = torch.where(torch.rand(run.shape, generator=g, device="cuda") < 0.33, torch.zeros_like(run), run)
    path = run.repeat_interleave(5, dim=0)[:T]                     # [T, S]
    y = torch.rand(T * S, K, generator=g, device="cuda") * (0.5 / K)
    y[torch.arange(T * S, device="cuda"), path.reshape(-1)] = 0.6
    refs = []
    p = path.cpu().numpy()
    for s in range(S):
        col = p[:lens[s], s]
        keep = (col != 0) & np.concatenate([[True], col[1:] != col[:-1]])
        lab = col[keep][:1023].copy()
        lab[::10] = 1 + (lab[::10] % (K - 1))
        refs.append(lab.tolist())
    return y, refs


def host_route(y, lens, S, blank=0):
    t0 = time.perf_counter()
    fc = y.cpu().numpy().argmax(1).reshape(-1, S)
    hyps = []
    for s in range(S):
        col = fc[:lens[s], s]
        keep = (col != blank) & np.concatenate([[True], col[1:] != col[:-1]])
        hyps.append(col[keep].tolist())
    return (time.perf_counter() - t0) * 1e6, hyps


def layer_forward(S, T, iters, warmup):
    rng = np.random.RandomState(S + T)
    x = torch.from_numpy(rng.randn(T * S, I).astype(np.float32)).cuda()
    ld = torch.tensor(lengths(S, T), dtype=torch.int32, device="cuda")
    bl = k.BidirectionalLstm(I, C, R, S)
    bl.set_params(rg.trained_params(I, C, R, 1), rg.trained_params(I, C, R, 2))
    out = torch.empty(T * S, 2 * R, device="cuda")
    us = timed(lambda: bl.propagate(x, ld, out), iters, warmup)
    bl.close()
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--call-only", action="store_true")
    ap.add_argument("--frames", default="300,1000,2000")
    ap.add_argument("--streams", default="4,8,32")
    ap.add_argument("--classes", default="48,1024,16624")
    a = ap.parse_args()
    rows = []
    for S in (int(v) for v in a.streams.split(",")):
        for T in (int(v) for v in a.frames.split(",")):
            if T * S > 65535:
                continue
            layer = None if a.call_only else layer_forward(S, T, max(2, a.iters // 2), max(1, a.warmup // 2))
            for K in (int(v) for v in a.classes.split(",")):
                g = torch.Generator(device="cuda").manual_seed(S * 7 + T + K)
                lens = lengths(S, T)
                y, refs = peaked(T, S, K, lens, g)
                ld = torch.tensor(lens, dtype=torch.int32, device="cuda")
                packed = k.ctc.pack_labels(refs, y.device)
                need = sum(lens) * K * 4
                r = {"T": T, "S": S, "K": K, "hyp_tokens": None, "ref_tokens": sum(len(x) for x in refs)}
                if a.call_only:
                    r["call_us"] = round(timed(lambda: k.ctc_greedy_decode(y, ld, 0, None, packed), a.iters, a.warmup), 1)
                    r["no_refs_us"] = round(timed(lambda: k.ctc_greedy_decode(y, ld, 0), a.iters, a.warmup), 1)
                else:
                    src = torch.empty(need // 4, device="cuda")
                    dst = torch.empty_like(src)
                    legs = {"call_us": lambda: k.ctc_greedy_decode(y, ld, 0, None, packed), "no_refs_us": lambda: k.ctc_greedy_decode(y, ld, 0),
                            "torch_argmax_us": lambda: torch.argmax(y, dim=1), "copy_us": lambda: dst.copy_(src)}
                    best = {}
                    for _ in range(3):                                   # alternating: three rounds, the fastest of each leg
                        for name, fn in legs.items():
                            us = timed(fn, a.iters, a.warmup)
                            best[name] = min(best.get(name, us), us)
                    r.update({n: round(v, 1) for n, v in best.items()})
                    r["host_us"], hyps = host_route(y, lens, S)
                    r["host_us"] = round(r["host_us"], 1)
                    res = k.ctc_greedy_decode(y, ld, 0, None, packed)
                    assert k.hypotheses_to_lists(res.hyp, res.hyp_len) == hyps, "the device and the host route disagree"
                    r["read_GBps"] = round(need / best["no_refs_us"] / 1e3, 1)
                    r["copy_GBps"] = round(need / best["copy_us"] / 1e3, 1)
                    r["call_over_torch_argmax"] = round(best["call_us"] / best["torch_argmax_us"], 3)
                    r["blstm_40_800_512_fwd_us"] = round(layer, 1)
                    r["call_share_of_layer_pct"] = round(100.0 * best["call_us"] / layer, 2)
                    del src, dst
                res = k.ctc_greedy_decode(y, ld, 0, None, packed)
                r["hyp_tokens"] = int(res.hyp_len.sum())
                r["errors"] = int(res.errors.sum())
                rows.append(r)
                print(json.dumps(r), flush=True)
                del y
    if a.call_only:
        print("\n    T   S      K   call us  no_refs us")
        for r in rows:
            print(f"{r['T']:5d} {r['S']:3d} {r['K']:6d} {r['call_us']:9.1f} {r['no_refs_us']:11.1f}")
        return
    print("\n    T   S      K   call us  no_refs  torch.argmax   call/argmax      host us  read GB/s  copy GB/s   layer fwd us   share")
    for r in rows:
        print(f"{r['T']:5d} {r['S']:3d} {r['K']:6d} {r['call_us']:9.1f} {r['no_refs_us']:8.1f} {r['torch_argmax_us']:13.1f} {r['call_over_torch_argmax']:13.3f} "
              f"{r['host_us']:12.1f} {r['read_GBps']:10.1f} {r['copy_GBps']:10.1f} {r['blstm_40_800_512_fwd_us']:14.1f} {r['call_share_of_layer_pct']:6.2f}%")


if __name__ == "__main__":
    main()
