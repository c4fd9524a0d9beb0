"""What the streaming CTC prefix beam search costs (klstm_ctc_beam_stream_step / _emit; profiles/ctc_beam_stream_probe.json):
device microseconds per frame of the longest utterance over T frames fed in chunks of 20 / 50 / 100, on the tensor, the ragged
lengths and the peaked posteriors of tools/ctc_beam_probe.py, next to the whole-utterance call on the same frames in the same process:
  whole          ctc_beam_decode without references (tools/ctc_beam_probe.py's "chain/frame" column)
  step           CtcBeamStream.step for every chunk: the row top-C and the search chain of the chunk, one state round trip
  step+emit      the same with an emit (1-best, mode 1) after EVERY chunk: partial results
  step+emit@end  the same with one emit after the last chunk
and, with --lm, a character bigram at K = 64 whose tables are staged into LDS again by every step, against the same automaton padded
with unreachable states until the tables are gathered from global memory: whether re-staging per chunk loses to the gather.
Chunks are row ranges of one tensor (no copies); lengths, start flags and modes are on the device before the clock starts.  Device
events around warmed-up repeats that end in a synchronise.  One JSON line per shape; --out writes them all as one JSON document.

    python tools/ctc_beam_stream_probe.py [--iters 3] [--warmup 1] [--frames 1000] [--streams 8,32] [--classes 64,16624]
                                          [--plans 4/4,16/8,64/32] [--chunks 20,50,100] [--lm] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kaldi_lstm_amd as k  # noqa: E402
from tools.ctc_decode_probe import lengths, peaked, timed  # noqa: E402


def stream_times(y, lens, S, K, T, B, C, chunks, iters, warmup, lm=None):
    """-> {chunk: (step, step + emit every chunk, step + emit at the end)} in microseconds per frame of the longest utterance"""
    out = {}
    bs = k.CtcBeamStream(S, K, T, beam=B, cands=C, lm=lm)
    mode = torch.ones(S, dtype=torch.int32, device="cuda")
    for c in chunks:
        plan = []
        for t0 in range(0, T, c):
            n = [max(0, min(c, v - t0)) for v in lens]
            plan.append((y[t0 * S:min(t0 + c, T) * S], torch.tensor(n, dtype=torch.int32, device="cuda"),
                         torch.full((S,), int(t0 == 0), dtype=torch.int32, device="cuda")))

        def run(every, end):
            for rows, n, st in plan:
                bs.step(rows, n, start=st)
                if every:
                    bs.emit(mode, nbest=1)
            if end:
                bs.emit(mode, nbest=1)
        f = float(max(lens))
        out[c] = tuple(round(timed(lambda e=e, d=d: run(e, d), iters, warmup) / f, 2) for e, d in ((False, False), (True, False), (False, True)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--streams", default="8,32")
    ap.add_argument("--classes", default="64,16624")
    ap.add_argument("--plans", default="4/4,16/8,64/32")
    ap.add_argument("--chunks", default="20,50,100")
    ap.add_argument("--lm", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ints = lambda v: [int(x) for x in v.split(",")]   # noqa: E731
    plans = [tuple(int(x) for x in p.split("/")) for p in a.plans.split(",")]
    chunks, T = ints(a.chunks), a.frames
    rows = []
    for S in ints(a.streams):
        for K in ints(a.classes):
            g = torch.Generator(device="cuda").manual_seed(S * 7 + T + K)
            lens = lengths(S, T)
            y, _ = peaked(T, S, K, lens, g)
            ld = torch.tensor(lens, dtype=torch.int32, device="cuda")
            for B, C in plans:
                r = {"T": T, "S": S, "K": K, "beam": B, "cands": C}
                r["whole_us_per_frame"] = round(timed(lambda: k.ctc_beam_decode(y, ld, 0, B, C, 1), a.iters, a.warmup) / max(lens), 2)
                for c, (st, every, end) in stream_times(y, lens, S, K, T, B, C, chunks, a.iters, a.warmup).items():
                    r[f"chunk{c}_step"], r[f"chunk{c}_step_emit_every"], r[f"chunk{c}_step_emit_end"] = st, every, end
                rows.append(r)
                print(json.dumps(r), flush=True)
            del y
    lm_rows = []
    if a.lm:
        K, B, C = 64, 16, 8
        rng = np.random.RandomState(3)
        nxt = np.tile(1 + np.arange(K, dtype=np.int32), (K + 1, 1))
        wt = np.exp(0.3 * rng.randn(K + 1, K)).astype(np.float32)
        q_big = K + 1
        while k.load_library().klstm_ctc_beam_lm_resident(q_big, K, B, C):
            q_big += 1
        pad = q_big - (K + 1)
        tables = {"resident": (nxt, wt), "gather": (np.concatenate([nxt, np.zeros((pad, K), np.int32)]), np.concatenate([wt, np.ones((pad, K), np.float32)]))}
        for S in ints(a.streams):
            g = torch.Generator(device="cuda").manual_seed(S * 7 + T + K)
            lens = lengths(S, T)
            y, _ = peaked(T, S, K, lens, g)
            ld = torch.tensor(lens, dtype=torch.int32, device="cuda")
            for where, (nx, w) in tables.items():
                lm = k.CtcLabelLm(nx, w)
                assert lm.resident(B, C) == (where == "resident")
                r = {"T": T, "S": S, "K": K, "beam": B, "cands": C, "lm_tables": where, "lm_bytes": int(nx.size * 8)}
                r["whole_us_per_frame"] = round(timed(lambda: k.ctc_beam_decode(y, ld, 0, B, C, 1, lm=lm), a.iters, a.warmup) / max(lens), 2)
                for c, (st, every, end) in stream_times(y, lens, S, K, T, B, C, chunks, a.iters, a.warmup, lm=lm).items():
                    r[f"chunk{c}_step"], r[f"chunk{c}_step_emit_every"], r[f"chunk{c}_step_emit_end"] = st, every, end
                lm_rows.append(r)
                print(json.dumps(r), flush=True)
    for title, table in (("no language model", rows), ("bigram at K = 64", lm_rows)):
        if not table:
            continue
        print(f"\n{title}: us per frame of the longest utterance ({T} frames)\n   S      K  B/C   " + ("tables   " if table is lm_rows else "") + "    whole " +
              "".join(f" {'step@%d' % c:>9s} {'+emit/chunk':>11s} {'+emit@end':>9s}" for c in chunks))
        for r in table:
            print(f"{r['S']:4d} {r['K']:6d} {r['beam']:2d}/{r['cands']:<2d} " + (f"{r['lm_tables']:>9s} " if table is lm_rows else "") + f"{r['whole_us_per_frame']:9.2f} " +
                  "".join(f" {r['chunk%d_step' % c]:9.2f} {r['chunk%d_step_emit_every' % c]:11.2f} {r['chunk%d_step_emit_end' % c]:9.2f}" for c in chunks))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"frames": T, "iters": a.iters, "warmup": a.warmup, "unit": "device microseconds per frame of the longest utterance",
                       "no_lm": rows, "bigram_k64": lm_rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
