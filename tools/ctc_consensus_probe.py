"""What MBR decoding and confidences cost next to the search that makes the lists: device time per call of ctc_nbest_consensus (five
launches: keys, distances, posteriors / risks / pivot, alignments, confidences / totals) and of ctc_beam_decode on the same batch.
S = 8 streams, T = 300 frames, peaked posteriors around references of 60 tokens in 12 words (class 1 separates them), K = 64;
N-best lists of N = 8, 16 and 64 entries (beam = max(16, N), 8 candidates); the consensus over tokens and over words.  Device events
around warmed-up repeats that end in a synchronise, the three legs alternating, TRIALS times; the median and the spread are kept.
The times are per CALL through the Python entry: they include its allocations and five (or the search's) launches, so at these sizes
they bound the kernels from above.  Writes profiles/ctc_consensus_probe.json (DESIGN.md 4r quotes it).

    python tools/ctc_consensus_probe.py [--iters 50] [--warmup 5] [--out profiles/ctc_consensus_probe.json]"""
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

S, T, K, WORDS, WORD_LEN, SEP, TRIALS = 8, 300, 64, 12, 4, 1, 5


def batch():
    g = torch.Generator(device="cuda").manual_seed(11)
    z = torch.randn(T, S, K, generator=g, device="cuda") * 0.7
    z[:, :, 0] += 3.0
    refs = []
    for s in range(S):
        lab = torch.randint(2, K, (WORDS * (WORD_LEN + 1) - 1,), generator=g, device="cuda")
        lab[WORD_LEN::WORD_LEN + 1] = SEP
        n = lab.numel()
        t = ((torch.arange(n, device="cuda") + 0.5) * T / n).long()
        z[t, s, lab] += 4.0
        refs.append(lab.tolist())
    return torch.softmax(z, -1).reshape(T * S, K).contiguous(), torch.full((S,), T, dtype=torch.int32, device="cuda"), refs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_consensus_probe.json"))
    a = ap.parse_args()
    y, lens, refs = batch()
    packed = k.ctc.pack_labels(refs, y.device)
    rows = []
    for N in (8, 16, 64):
        beam = max(16, N)

        def search():
            return k.ctc_beam_decode(y, lens, beam=beam, cands=8, nbest=N, refs=packed)
        nb = search()
        legs = {"beam_us": search, "consensus_tokens_us": lambda: k.ctc_nbest_consensus(nb), "consensus_words_us": lambda: k.ctc_nbest_consensus(nb, separator=SEP)}
        times = {name: [] for name in legs}
        for _ in range(TRIALS):
            for name, leg in legs.items():
                times[name].append(timed(leg, a.iters, a.warmup))
        totals = torch.zeros(10, dtype=torch.float64, device="cuda")
        tok = k.ctc_nbest_consensus(nb, totals=totals)
        wtotals = torch.zeros(10, dtype=torch.float64, device="cuda")
        wrd = k.ctc_nbest_consensus(nb, separator=SEP, totals=wtotals)
        t, w = totals.cpu().tolist(), wtotals.cpu().tolist()
        assert t[0] == S and w[0] == S and bool((tok.pick >= 0).all()) and bool((wrd.pick >= 0).all())
        r = {"S": S, "T": T, "K": K, "N": N, "beam": beam, "entries_listed": int(nb.nbest_count.sum()),
             "tokens_per_entry": round(float(nb.hyp_len.sum()) / max(1, int(nb.nbest_count.sum())), 1), "words_per_pick": w[5] / S,
             "expected_token_errors_mbr": t[2] / S, "expected_token_errors_map": t[3] / S, "streams_mbr_differs": int(t[4]),
             "mean_token_confidence": t[6] / t[5], "mean_word_confidence": w[6] / w[5],
             "workspace_bytes_tokens": k.ctc_consensus_workspace_bytes(S, N, min(1023, T), False),
             "workspace_bytes_words": k.ctc_consensus_workspace_bytes(S, N, min(1023, T), True)}
        for name, v in times.items():
            r[name] = round(statistics.median(v), 1)
            r[name + "_min_max"] = [round(min(v), 1), round(max(v), 1)]
        r["consensus_tokens_over_beam"] = round(r["consensus_tokens_us"] / r["beam_us"], 4)
        rows.append(r)
        print(json.dumps(r), flush=True)
    out = {"what": "device microseconds per call through the Python entries, median of %d trials of %d calls; S = 8, T = 300, about 60 tokens in 12 words" % (TRIALS, a.iters),
           "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
