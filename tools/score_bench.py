"""Timing of batched scoring (include/klstm_scorer.hpp) at the configs[3] topology: Transmit -> LstmProjectedStreams 40 -> 512 ->
LstmProjectedStreams 512 -> 512 (cell 800) -> AffineTransform 16624 -> Softmax, 64 utterances of 200..1200 frames.

  (a) frames/s of the per-utterance path (nnet-forward: S = 1 engines, one utterance per call, whole utterance, Affine, Softmax)
      against the scorer's launch sequence at S = 4 / 8 / 16 (pack -> propagate_inference per layer -> affine -> log_softmax_scatter
      per chunk, the plan of klstm_scorer.hpp PlanChunks), for each chunk length T in --chunks;
  (b) forward-chain microseconds per chunk of klstm_propagate against klstm_propagate_inference at S = 1, 4, 5, 8, 12, 16 and
      T = 20, 50 (the 40 -> 800 -> 512 layer and the 512 -> 800 -> 512 layer), the two calls alternating in the same run, with the
      engine's count of forward-only (INF) launches: where it is 0 both calls run the same kernels;
  (c) where the time of the scorer goes at S = 16 (--breakdown-chunk, default 50): each stage of the chunk loop timed in a loop of
      its own (pack, layer 1 chain, layer 2 chain, Affine, output kernel), the loop without the per-call host wait of
      "persist_verify" = 1, and the fraction of padding rows in the plan; S = 8 the same for comparison.

HIP events around synchronised work, on the library's stream (engines created without a stream; the stateless calls go to the
legacy default stream, which that stream is ordered with).  Prints one JSON object.  Usage: python tools/score_bench.py [--chunks 20,50,100]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import kaldi_lstm_amd as k  # noqa: E402

I, C, R, NPDF = 40, 800, 512, 16624


def plan(lens, S, T):
    """klstm_scorer.hpp PlanChunks restated: (desc [S, 3], reset [S], dst [T*S]) per chunk"""
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    queue = [u for u in range(len(lens)) if lens[u] > 0]
    utt, cur, chunks = [None] * S, [0] * S, []
    while True:
        for s in range(S):
            if utt[s] is None or cur[s] >= lens[utt[s]]:
                utt[s], cur[s] = (queue.pop(0) if queue else None), 0
        if all(u is None for u in utt):
            return chunks
        desc, reset, dst = np.zeros((S, 3), np.int32), np.ones(S, np.int32), -np.ones((T, S), np.int32)
        for s in range(S):
            if utt[s] is None:
                continue
            u, n = utt[s], lens[utt[s]]
            desc[s] = (off[u], n, cur[s]); reset[s] = int(cur[s] == 0)
            t = np.arange(T)
            dst[:, s] = np.where(cur[s] + t < n, off[u] + cur[s] + t, -1)
            cur[s] += T
        chunks.append((desc, reset, dst.ravel()))


def timed(fn, reps=1):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps         # ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", default="20,50,100")
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--breakdown-chunk", type=int, default=50)
    args = ap.parse_args()
    rng = np.random.RandomState(0)
    flats = [rng.uniform(-0.1, 0.1, 4 * C * i + 4 * C * R + 4 * C + 3 * C + R * C).astype(np.float32) for i in (I, R)]
    W = torch.from_numpy(rng.uniform(-0.1, 0.1, (NPDF, R)).astype(np.float32)).cuda()
    b = torch.from_numpy(rng.uniform(-0.1, 0.1, NPDF).astype(np.float32)).cuda()
    lens = rng.randint(200, 1201, args.utts)
    feats = torch.from_numpy(rng.uniform(-1, 1, (int(lens.sum()), I)).astype(np.float32)).cuda()
    out = torch.empty(int(lens.sum()), NPDF, device="cuda")
    frames = float(lens.sum())
    res = {"topology": "Transmit -> 40-800-512 -> 512-800-512 -> Affine 16624 -> Softmax", "utterances": int(args.utts),
           "frames": int(frames), "a_frames_per_s": {}, "b_us_per_chunk": {}, "c_breakdown": {}}

    # ---- (a) per utterance, S = 1: what the nnet-forward workalike runs (LstmProjected resets per utterance, whole utterance per call)
    e1 = [k.Engine(I if l == 0 else R, C, R, 1) for l in range(2)]
    for e, f in zip(e1, flats):
        e.set_params(f); e.set_option("persist_verify", 1)
    nmax = int(lens.max())
    h = [torch.empty(nmax, R, device="cuda") for _ in range(2)]
    a1 = torch.empty(nmax, NPDF, device="cuda")
    offs = np.concatenate([[0], np.cumsum(lens)])

    def per_utt():
        for u, n in enumerate(lens):
            x = feats[offs[u]:offs[u] + n]
            for l, e in enumerate(e1):
                e.reset([1])
                e.propagate(x if l == 0 else h[l - 1][:n], h[l][:n])
            k.affine_propagate(h[1][:n], W, b, a1[:n])
            k.softmax(a1[:n], out[offs[u]:offs[u] + n])
    per_utt()
    ms = min(timed(per_utt) for _ in range(args.reps))
    res["a_frames_per_s"]["per_utterance_S1"] = frames / ms * 1e3
    for e in e1:
        e.close()

    # ---- (a) the scorer at S = 4 / 8 / 16, (c) the breakdown
    def setup(S, T, verify=1):
        es = [k.Engine(I if l == 0 else R, C, R, S) for l in range(2)]
        for e, f in zip(es, flats):
            e.set_params(f); e.set_option("persist_verify", verify)
        p = plan(lens, S, T)
        st = dict(es=es, p=p, descs=torch.from_numpy(np.stack([c[0] for c in p])).cuda(),
                  dsts=torch.from_numpy(np.stack([c[2] for c in p])).cuda(), x0=torch.empty(T * S, I, device="cuda"),
                  hs=[torch.empty(T * S, R, device="cuda") for _ in range(2)], a=torch.empty(T * S, NPDF, device="cuda"))
        return st

    def stages(st, S, T, which=("pack", "lstm1", "lstm2", "affine", "output")):
        es, p, x0, hs, a = st["es"], st["p"], st["x0"], st["hs"], st["a"]
        for c, (_, reset, _) in enumerate(p):
            if "pack" in which:
                k.pack_streams(feats, st["descs"][c], T, 0, x0)
            for l, e in enumerate(es):
                if "lstm%d" % (l + 1) in which:
                    e.reset(reset)
                    e.propagate_inference(x0 if l == 0 else hs[l - 1], hs[l])
            if "affine" in which:
                k.affine_propagate(hs[1], W, b, a)
            if "output" in which:
                k.log_softmax_scatter(a, st["dsts"][c], out, k.SCORE_POSTERIOR)

    for T in [int(t) for t in args.chunks.split(",")]:
        for S in (4, 8, 16):
            st = setup(S, T)
            stages(st, S, T)
            ms = min(timed(lambda: stages(st, S, T)) for _ in range(args.reps))
            res["a_frames_per_s"]["scorer_S%d_T%d" % (S, T)] = frames / ms * 1e3
            for e in st["es"]:
                e.close()
    T = args.breakdown_chunk
    for S in (8, 16):
        st = setup(S, T)
        stages(st, S, T)
        br = {"whole_ms": min(timed(lambda: stages(st, S, T)) for _ in range(args.reps))}
        for w in ("pack", "lstm1", "lstm2", "affine", "output"):
            br[w + "_ms"] = min(timed(lambda: stages(st, S, T, (w,))) for _ in range(args.reps))
        br["chunks"] = len(st["p"])
        br["padding_row_fraction"] = 1.0 - frames / (len(st["p"]) * T * S)
        br["fwd_inference_launches"] = [e.profile_query("fwd_inference_launches")[1] for e in st["es"]]
        for e in st["es"]:
            e.close()
        st = setup(S, T, verify=0)
        stages(st, S, T)
        br["whole_ms_persist_verify_0"] = min(timed(lambda: stages(st, S, T)) for _ in range(args.reps))
        for e in st["es"]:
            e.close()
        res["c_breakdown"]["S%d_T%d" % (S, T)] = br

    # ---- (b) forward chain per chunk: klstm_propagate vs klstm_propagate_inference, alternating
    for (li, name) in ((I, "40-800-512"), (R, "512-800-512")):
        for S in (1, 4, 5, 8, 12, 16):
            for T in (20, 50):
                e = k.Engine(li, C, R, S)
                e.set_params(flats[0] if li == I else flats[1])
                x = torch.from_numpy(rng.uniform(-1, 1, (T * S, li)).astype(np.float32)).cuda()
                o = torch.empty(T * S, R, device="cuda")
                for _ in range(20):
                    e.propagate(x, o); e.propagate_inference(x, o)
                tr, ti = [], []
                for _ in range(10):
                    tr.append(timed(lambda: e.propagate(x, o), 50))
                    ti.append(timed(lambda: e.propagate_inference(x, o), 50))
                res["b_us_per_chunk"]["%s_S%d_T%d" % (name, S, T)] = {
                    "propagate": 1e3 * float(np.median(tr)), "propagate_inference": 1e3 * float(np.median(ti)),
                    "fwd_inference_launches": e.profile_query("fwd_inference_launches")[1]}
                e.close()
    best = max(v for kk, v in res["a_frames_per_s"].items() if kk.startswith("scorer_S16"))
    res["a_speedup_S16_over_per_utterance"] = best / res["a_frames_per_s"]["per_utterance_S1"]
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
