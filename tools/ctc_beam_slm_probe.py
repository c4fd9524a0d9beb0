"""What a sparse back-off language model costs the CTC prefix beam search (klstm_ctc_beam_decode_slm; DESIGN.md 4q;
profiles/ctc_beam_slm_probe.txt): device time per frame of the search chain at T = 1000, K = 64 on the peaked posteriors of
tools/ctc_decode_probe.py (all streams of full length, so the time of the call is the time of one chain), without references, for
  none            ctc_beam_decode without an LM
  bigram, order5  the sparse call on an absolute-discounting back-off model of that order (lm.backoff_ngram_label_lm on sequences of a
                  random second-order chain)
  *_dense         the dense call on the expansion of the same model (lm.sparse_lm_to_dense), padded with unreachable states past the
                  LDS threshold so that it GATHERS its tables from global memory, as the sparse call must: the same bits, the fair pair
  bigram_lds      the dense call on the bigram's expansion as it is: 33 KB, resident in LDS
and beam / candidates 4/4, 16/8, 64/32.  Every figure is the MEDIAN over --repeats timings of --iters calls each (device events around
warmed-up calls that end in a synchronise), with the spread (max - min) / median of those timings next to it.  --depth-frames n > 0
also runs the numpy twin on the first n frames of stream 0 and reports what share of the lookups backed off how far.  One JSON line
per shape and a table at the end.  The comparison with the commit before the feature is tools/ctc_beam_lm_probe.py run from both
trees in turn: it times the LM-less call and the two dense plans, which this feature must leave as they were.

    python tools/ctc_beam_slm_probe.py [--iters 5] [--warmup 2] [--repeats 5] [--frames 1000] [--streams 1,8,32] [--classes 64]
                                       [--configs 4/4,16/8,64/32] [--depth-frames 60] [--setups none,bigram,...]

Another layout rule is another build of the same sources (-DKLSTM_SLM_DIRECT_DIV=0: no direct rows, every lookup a binary search),
loaded through KLSTM_LIB_PATH."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kaldi_lstm_amd as k  # noqa: E402
from tests import ctc_beam_slm_ref as R  # noqa: E402
from tools.ctc_decode_probe import peaked, timed  # noqa: E402

SETUPS = ["none", "bigram_lds", "bigram_dense", "bigram", "order5_dense", "order5"]


def gathered(dense, K, B, C):
    """the dense tables padded with unreachable states until a call of this shape gathers them"""
    nxt, wt, fin = dense
    Q = nxt.shape[0]
    while k.load_library().klstm_ctc_beam_lm_resident(Q, K, B, C):
        Q += 16
    pad = Q - nxt.shape[0]
    return k.CtcLabelLm(np.concatenate([nxt, np.zeros((pad, K), np.int32)]), np.concatenate([wt, np.zeros((pad, K), np.float32)]),
                        np.concatenate([fin, np.zeros(pad, np.float32)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", default="1000")
    ap.add_argument("--streams", default="1,8,32")
    ap.add_argument("--classes", default="64")
    ap.add_argument("--configs", default="4/4,16/8,64/32")
    ap.add_argument("--depth-frames", type=int, default=60)
    ap.add_argument("--setups", default=",".join(SETUPS))
    a = ap.parse_args()
    setups = a.setups.split(",")
    ints = lambda v: [int(x) for x in v.split(",")]   # noqa: E731
    configs = [tuple(int(x) for x in v.split("/")) for v in a.configs.split(",")]
    rows = []
    for K in ints(a.classes):
        seqs = R.markov_sequences(np.random.RandomState(K), K, 0, 400, 12)
        models = {name: k.backoff_ngram_label_lm(seqs, K, 0, order=order, alpha=0.8, beta=0.5) for name, order in (("bigram", 2), ("order5", 5))}
        dense = {name: k.sparse_lm_to_dense(m) for name, m in models.items()}
        sparse = {name: k.CtcSparseLabelLm(m, 0) for name, m in models.items()}
        for name, m in models.items():
            st = sparse[name].status_list()
            print(json.dumps({"model": name, "K": K, "states": len(m.backoff), "arcs": len(m.arc_labels), "blob_bytes": sparse[name].nbytes,
                              "dense_bytes": dense[name][0].size * 8, "direct_rows": st[6], "dropped_or_cut": sum(st[:6])}), flush=True)
        for S in ints(a.streams):
            for T in ints(a.frames):
                if T * S > 65535:
                    continue
                g = torch.Generator(device="cuda").manual_seed(S * 7 + T + K)
                lens = [T] * S
                y, _ = peaked(T, S, K, lens, g)
                ld = torch.tensor(lens, dtype=torch.int32, device="cuda")
                for B, C in configs:
                    lms = {"none": None, "bigram_lds": k.CtcLabelLm(*dense["bigram"]), "bigram": sparse["bigram"], "order5": sparse["order5"],
                           "bigram_dense": gathered(dense["bigram"], K, B, C), "order5_dense": gathered(dense["order5"], K, B, C)}
                    assert lms["bigram_lds"].resident(B, C) and not lms["bigram_dense"].resident(B, C) and not lms["order5_dense"].resident(B, C)
                    r = {"T": T, "S": S, "K": K, "beam": B, "cands": C}
                    out = {}
                    for s in setups:
                        kw = {} if s == "none" else {"lm": lms[s]}
                        ts = [timed(lambda: k.ctc_beam_decode(y, ld, 0, B, C, min(B, 4), **kw), a.iters, a.warmup if i == 0 else 0)
                              for i in range(a.repeats)]
                        med = statistics.median(ts)
                        r[s + "_us_per_frame"] = round(med / T, 3)
                        r[s + "_spread"] = round((max(ts) - min(ts)) / med, 4)
                        out[s] = k.ctc_beam_decode(y, ld, 0, B, C, min(B, 4), **kw)
                    torch.cuda.synchronize()
                    for name in models:                           # the pair computes the same bits
                        if name not in out or name + "_dense" not in out:
                            continue
                        x, z = out[name], out[name + "_dense"]
                        r[name + "_bits_equal"] = bool(torch.equal(x.nbest_count, z.nbest_count) and
                                                       torch.equal(x.score[:, 0].view(torch.int32), z.score[:, 0].view(torch.int32)))
                    if a.depth_frames > 0 and S == ints(a.streams)[0]:
                        n = min(a.depth_frames, T)
                        yh = y.cpu().numpy().reshape(T, S, K)[:n, :1]
                        for name, m in models.items():
                            _, tabs = R.beam_twin_slm(yh, [n], 0, B, C, 1, m, lazy=True)
                            total = sum(tabs.reads.values())
                            r[name + "_depth_share"] = [round(tabs.reads[d] / total, 3) for d in range(max(tabs.reads) + 1)]
                    rows.append(r)
                    print(json.dumps(r), flush=True)
                del y
    print("\n    T   S   K  beam/cands " + "".join(f" {s:>13s} {'spread':>7s}" for s in setups) + "   (us per frame)")
    for r in rows:
        print(f"{r['T']:5d} {r['S']:3d} {r['K']:3d} {'%d/%d' % (r['beam'], r['cands']):>11s} " +
              "".join(f" {r[s + '_us_per_frame']:13.3f} {100 * r[s + '_spread']:6.1f}%" for s in setups))


if __name__ == "__main__":
    main()
