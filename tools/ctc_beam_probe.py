"""What CTC prefix beam search costs (klstm_ctc_beam_decode; profiles/ctc_beam_probe.txt): device time of the whole call --
row top-C, the search chain, hypotheses, scores, edit distances -- at the shapes of tools/ctc_decode_probe.py with its ragged lengths
and its peaked posteriors, for beam B in {4, 16, 64} x candidates C in {4, 8, 32}, next to its yardsticks on the same tensor in the
same process:
  greedy         ctc_greedy_decode with references (klstm_ctc_decode, the best path): what a user had before
  beam B/C       ctc_beam_decode with references, 4-best
  chain/frame    the same call WITHOUT references over the longest utterance's frames: an UPPER bound of the search chain's time per
                 frame (it still holds the top-C launch and two launch overheads; at K = 48 the top-C launch is a few microseconds)
  topc (K=16624) the call at K = 16624 minus the call at K = 48 with the same T, S, B, C: the search chain does not depend on K, so the
                 difference is the top-C launch over the big rows -- an ESTIMATE by subtraction, next to torch.topk(net_out, C, dim=1)
                 on the same tensor (which reads the padding rows too and does none of the rest)
Device events around warmed-up repeats that end in a synchronise.  One JSON line per shape and a table at the end.

    python tools/ctc_beam_probe.py [--iters 5] [--warmup 2] [--call-only] [--frames 300,1000] [--streams 4,32] [--classes 48,1024,16624]
                                   [--beams 4,16,64] [--cands 4,8,32]

--call-only: the beam call without references only, no yardsticks (a rocprofv3 --kernel-trace --stats run; geometry comparisons)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kaldi_lstm_amd as k  # noqa: E402
from tools.ctc_decode_probe import lengths, peaked, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--call-only", action="store_true")
    ap.add_argument("--frames", default="300,1000")
    ap.add_argument("--streams", default="4,32")
    ap.add_argument("--classes", default="48,1024,16624")
    ap.add_argument("--beams", default="4,16,64")
    ap.add_argument("--cands", default="4,8,32")
    a = ap.parse_args()
    ints = lambda v: [int(x) for x in v.split(",")]   # noqa: E731
    rows = []
    for S in ints(a.streams):
        for T in ints(a.frames):
            if T * S > 65535:
                continue
            small = {}                                                   # (B, C) -> no-refs time at the smallest K of this (T, S)
            for K in sorted(ints(a.classes)):
                g = torch.Generator(device="cuda").manual_seed(S * 7 + T + K)
                lens = lengths(S, T)
                y, refs = peaked(T, S, K, lens, g)
                ld = torch.tensor(lens, dtype=torch.int32, device="cuda")
                packed = k.ctc.pack_labels(refs, y.device)
                r = {"T": T, "S": S, "K": K, "ref_tokens": sum(len(x) for x in refs)}
                if not a.call_only:
                    r["greedy_us"] = round(timed(lambda: k.ctc_greedy_decode(y, ld, 0, None, packed), a.iters, a.warmup), 1)
                    g0 = k.ctc_greedy_decode(y, ld, 0, None, packed)
                    r["greedy_errors"] = int(g0.errors.sum())
                for B in ints(a.beams):
                    for C in ints(a.cands):
                        if C > K - 1:
                            continue
                        N = min(B, 4)
                        tag = f"b{B}c{C}"
                        norefs = timed(lambda: k.ctc_beam_decode(y, ld, 0, B, C, N), a.iters, a.warmup)
                        r[tag + "_norefs_us"] = round(norefs, 1)
                        r[tag + "_chain_us_per_frame"] = round(norefs / max(lens), 2)
                        if a.call_only:
                            continue
                        r[tag + "_us"] = round(timed(lambda: k.ctc_beam_decode(y, ld, 0, B, C, N, None, packed), a.iters, a.warmup), 1)
                        r[tag + "_over_greedy"] = round(r[tag + "_us"] / r["greedy_us"], 2)
                        res = k.ctc_beam_decode(y, ld, 0, B, C, N, None, packed)
                        r[tag + "_errors"] = int(res.errors[:, 0].sum())
                        r[tag + "_oracle_errors"] = int(torch.where(res.errors >= 0, res.errors, torch.full_like(res.errors, 1 << 20)).min(dim=1).values.sum())
                        small.setdefault((B, C), norefs)
                        if K == 16624:
                            r[tag + "_topc_est_us"] = round(norefs - small[(B, C)], 1)
                if K == 16624 and not a.call_only:
                    for C in ints(a.cands):
                        r[f"torch_topk{C}_us"] = round(timed(lambda: torch.topk(y, C, dim=1), a.iters, a.warmup), 1)
                rows.append(r)
                print(json.dumps(r), flush=True)
                del y
    Bs, Cs = ints(a.beams), ints(a.cands)
    key = "_norefs_us" if a.call_only else "_us"
    print("\n    T   S      K " + ("" if a.call_only else "   greedy") + "".join(f" {'b%dc%d' % (B, C):>9s}" for B in Bs for C in Cs) + "     (us per call" +
          (", no references)" if a.call_only else ", with references)"))
    for r in rows:
        print(f"{r['T']:5d} {r['S']:3d} {r['K']:6d} " + ("" if a.call_only else f"{r['greedy_us']:9.1f}") +
              "".join(f" {r.get('b%dc%d' % (B, C) + key, float('nan')):9.1f}" for B in Bs for C in Cs))
    print("\n    T   S      K " + "".join(f" {'b%dc%d' % (B, C):>9s}" for B in Bs for C in Cs) + "     (us per frame of the longest utterance, no references)")
    for r in rows:
        print(f"{r['T']:5d} {r['S']:3d} {r['K']:6d} " + "".join(f" {r.get('b%dc%d_chain_us_per_frame' % (B, C), float('nan')):9.2f}" for B in Bs for C in Cs))
    if not a.call_only:
        print("\n    T   S " + "".join(f" {'topc C=%d' % C:>10s} {'topk C=%d' % C:>10s}" for C in Cs) + "     (K = 16624: top-C launch, estimated with beam " +
              f"{Bs[0]}, against torch.topk, us)")
        for r in rows:
            if r["K"] == 16624:
                print(f"{r['T']:5d} {r['S']:3d} " + "".join(f" {r.get('b%dc%d_topc_est_us' % (Bs[0], C), float('nan')):10.1f} {r.get('torch_topk%d_us' % C, float('nan')):10.1f}"
                                                          for C in Cs))


if __name__ == "__main__":
    main()
