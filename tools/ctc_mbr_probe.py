"""What minimum expected token error training costs per minibatch: device time of the fused klstm_ctc_mbr_eval (the chains of every list
entry side by side, the weights on the device, the row written once) next to
  - the beam search that makes its lists (klstm_ctc_beam_decode, beam 16, 8 candidates, N-best),
  - the COMPOSITION a user of the library would write without it: N + 1 calls of klstm_ctc_eval (every list entry and the reference as
    the labels), the read-back of the N losses to the host for the weights, and N + 1 torch accumulate passes over the [T*S, K] diffs.
    Packing the lists into label arrays is left out of its time,
  - one bidirectional LSTMP layer's forward + BPTT at 40/800/512 with the same S and T, as tools/ctc_probe.py times it,
on the (S, T, L, K) grid of tools/ctc_probe.py with N = 4 and 8, peaked posteriors around references of L labels (the lists then hold
labellings of about L labels), risk scale 1, CTC weight 0.3.  Device events around warmed-up repeats that end in a synchronise, all
legs in the same process.  Prints one JSON line per shape and a table at the end (DESIGN.md 4n records it;
profiles/ctc_mbr_probe.txt).

    python tools/ctc_mbr_probe.py [--iters 10] [--warmup 3] [--mbr-only] [--small]

--mbr-only: the fused call alone (a rocprofv3 --kernel-trace --stats run of it); --small: S = 8 and 16 at T = 500 only."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kaldi_lstm_amd as k  # noqa: E402
from tools.ctc_probe import layer_leg, lengths, timed  # noqa: E402

KAPPA, LAM = 1.0, 0.3


def peaked(S, T, L, K):
    g = torch.Generator(device="cuda").manual_seed(S * 7 + T + L + K)
    lens, labs = lengths(S, T, L)
    labs[0] = L
    z = torch.randn(T, S, K, generator=g, device="cuda") * 0.5
    z[:, :, 0] += 2.4
    refs = []
    for s, n in enumerate(labs):
        lab = torch.randint(1, K, (n,), generator=g, device="cuda")
        t = ((torch.arange(n, device="cuda") + 0.5) * lens[s] / n).long()
        z[t, s, lab] += 4.0
        refs.append(lab.tolist())
    return torch.softmax(z, -1).reshape(T * S, K).contiguous(), lens, refs


def legs(S, T, L, K, N, iters, warmup, mbr_only):
    y, lens, refs = peaked(S, T, L, K)
    ld = torch.tensor(lens, dtype=torch.int32, device="cuda")
    packed_refs = k.ctc.pack_labels(refs, y.device)
    beam = k.ctc_beam_decode(y, ld, beam=16, cands=8, nbest=N, refs=packed_refs)
    lists = k.nbest_to_lists(beam)
    longest = max(len(h) for l in lists for h, _, _ in l)
    max_len = min(1023, max(longest, L) + 8)
    diff = torch.empty_like(y)
    fused = timed(lambda: k.ctc_mbr_eval(y, ld, beam, refs=packed_refs, risk_scale=KAPPA, ctc_weight=LAM, max_len=max_len, diff=diff), iters, warmup)
    res = k.ctc_mbr_eval(y, ld, beam, refs=packed_refs, risk_scale=KAPPA, ctc_weight=LAM, max_len=max_len, diff=diff)
    assert bool((res.risk >= 0).all()) and bool(torch.isfinite(res.diff).all())
    out = {"mbr_us": round(fused, 1), "workspace_mb": round(k.ctc_mbr_workspace_bytes(T, S, N, max_len, True) / 2 ** 20, 1), "max_len": max_len,
           "list_labels": int(sum(len(h) for l in lists for h, _, _ in l) / S)}
    if mbr_only:
        return out
    out["beam_us"] = round(timed(lambda: k.ctc_beam_decode(y, ld, beam=16, cands=8, nbest=N, refs=packed_refs), iters, warmup), 1)
    # the composition of the library's other entries
    packed = [k.ctc.pack_labels([l[q][0] if q < len(l) else [] for l in lists], y.device) for q in range(N)]
    listed = torch.tensor([[q < len(l) for q in range(N)] for l in lists], device="cuda")
    cost = beam.errors.double()
    total = torch.empty_like(y)
    S_of_row = torch.arange(T * S, device="cuda") % S

    def composition():
        losses = []
        k.ctc_eval(y, ld, packed_refs, 0, total)
        parts = []
        for q in range(N):
            loss, d = k.ctc_eval(y, ld, packed[q], 0, torch.empty_like(y))
            losses.append(loss)
            parts.append(d)
        lp = -torch.stack(losses, 1).cpu().double()                     # the host round trip: the weights need every loss
        lp[~listed.cpu()] = -float("inf")
        P = torch.softmax(KAPPA * lp, 1)
        W = cost.cpu()
        R = (P * W).sum(1, keepdim=True)
        c = (KAPPA * P * (W - R)).float().cuda()                        # [S, N]
        total.mul_(LAM)
        for q in range(N):
            total.addcmul_(parts[q], c[S_of_row, q][:, None], value=-1.0)      # sum_q c_q = 0: the y terms cancel
        return total, R
    comp = timed(composition, iters, warmup)
    tot, R = composition()
    torch.cuda.synchronize()
    out["composition_us"] = round(comp, 1)
    out["fused_vs_composition_max_abs"] = float((tot - res.diff).abs().max())
    out["speedup"] = round(comp / fused, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mbr-only", action="store_true")
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    rows = []
    for S in ((8, 16) if a.small else (8, 16, 32)):
        for T in ((500,) if a.small else (500, 1000)):
            layer = None if a.mbr_only else layer_leg(S, T, max(2, a.iters // 2), max(1, a.warmup // 2))[0]
            for K in (64, 4096):
                for L in (50, 150):
                    for N in (4, 8):
                        r = {"S": S, "T": T, "L": L, "K": K, "N": N}
                        r.update(legs(S, T, L, K, N, a.iters, a.warmup, a.mbr_only))
                        r["blstm_40_800_512_fwd_bptt_us"] = None if layer is None else round(layer, 1)
                        rows.append(r)
                        print(json.dumps(r), flush=True)
                        torch.cuda.empty_cache()
    print("\n  S     T    L     K  N    mbr us   beam us  composition us  speedup   layer us   ws MB")
    for r in rows:
        lay = r["blstm_40_800_512_fwd_bptt_us"]
        print(f"{r['S']:3d} {r['T']:5d} {r['L']:4d} {r['K']:5d} {r['N']:2d} {r['mbr_us']:9.1f} " +
              (f"{r['beam_us']:9.1f} {r['composition_us']:15.1f} {r['speedup']:8.2f} {lay:10.1f}" if lay is not None else " " * 46) +
              f" {r['workspace_mb']:7.1f}")


if __name__ == "__main__":
    main()
