"""What second-pass rescoring costs next to the search that makes the lists: device time per call of ctc_nbest_rescore (two launches: one
wave per entry walks the models, one wave per stream ranks and gathers) and of the ctc_beam_decode call that produced the lists, in
the same run.  Lists of about 100 and 300 tokens per entry (T = 3 tokens' worth of frames, peaked posteriors around sentences of
4-token words, class 1 the separator, K = 32), N = 8 and 64 entries, S = 1 and 32 streams; the first pass fuses a token bigram
(beam = max(16, N), 8 candidates).  Three second passes, each taking the bigram out: a token bigram, a token order-5 model, a word
trigram through a table of 200 words.  Device events around warmed-up repeats that end in a synchronise, the legs alternating, TRIALS
times; the median and the spread are kept.  The times are per CALL through the Python entry: they include its allocations and
launches, so at these sizes they bound the kernels from above.  Writes profiles/ctc_rescore_probe.json (DESIGN.md 4s quotes it).

    python tools/ctc_rescore_probe.py [--iters 20] [--warmup 3] [--out profiles/ctc_rescore_probe.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import kaldi_lstm_amd as k  # noqa: E402
from tools.ctc_probe import timed  # noqa: E402

K, SEP, WORD_LEN, VOCAB, TRIALS = 32, 1, 4, 200, 3


def language(seed=5):
    """a vocabulary, sentences with structure, and the three models"""
    rng = np.random.default_rng(seed)
    vocab = []
    while len(vocab) < VOCAB:
        w = rng.integers(2, K, size=WORD_LEN).tolist()
        if w not in vocab:
            vocab.append(w)
    fav = rng.integers(0, VOCAB, size=(VOCAB, 4))
    sents = []
    for _ in range(300):
        i = int(rng.integers(0, VOCAB))
        snt = [i]
        for _ in range(60):
            i = int(fav[i, rng.integers(0, 4)]) if rng.random() < 0.85 else int(rng.integers(0, VOCAB))
            snt.append(i)
        sents.append(snt)
    toks = [sum((vocab[i] + [SEP] for i in snt), [])[:-1] for snt in sents]
    table = k.word_table(vocab, SEP)
    unk, reserved, V = VOCAB, VOCAB + 1, VOCAB + 2
    word_seqs = k.word_sequences(toks, table, SEP, unk)
    return dict(sents=toks, table=table, unk=unk,
                bigram=k.CtcSparseLabelLm(k.backoff_ngram_label_lm(toks, K, 0, order=2), 0),
                order5=k.CtcSparseLabelLm(k.backoff_ngram_label_lm(toks, K, 0, order=5), 0),
                word3=k.CtcSparseLabelLm(k.backoff_ngram_label_lm(word_seqs, V, reserved, order=3), reserved))


def batch(sents, S, L):
    T = 3 * L
    g = torch.Generator(device="cuda").manual_seed(11)
    z = torch.randn(T, S, K, generator=g, device="cuda") * 0.7
    z[:, :, 0] += 3.0
    refs = []
    for s in range(S):
        lab = torch.tensor(sents[s][:L], device="cuda")
        t = ((torch.arange(L, device="cuda") + 0.5) * T / L).long()
        z[t, s, lab] += 9.0
        refs.append(lab.tolist())
    return torch.softmax(z, -1).reshape(T * S, K).contiguous(), torch.full((S,), T, dtype=torch.int32, device="cuda"), refs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_rescore_probe.json"))
    a = ap.parse_args()
    lang = language()
    words = k.CtcWordTable(*lang["table"], lang["unk"], SEP)
    rows = []
    for L in (100, 300):
        for S in (1, 32):
            y, lens, refs = batch(lang["sents"], S, L)
            packed = k.ctc.pack_labels(refs, y.device)
            for N in (8, 64):
                beam = max(16, N)

                def search():
                    return k.ctc_beam_decode(y, lens, beam=beam, cands=8, nbest=N, refs=packed, lm=lang["bigram"])
                nb = search()
                legs = {"beam_us": search,
                        "rescore_bigram_us": lambda: k.ctc_nbest_rescore(nb, add=lang["bigram"], sub=lang["bigram"]),
                        "rescore_order5_us": lambda: k.ctc_nbest_rescore(nb, add=lang["order5"], sub=lang["bigram"]),
                        "rescore_word3_us": lambda: k.ctc_nbest_rescore(nb, add=lang["word3"], sub=lang["bigram"], words=words)}
                times = {name: [] for name in legs}
                for _ in range(TRIALS):
                    for name, leg in legs.items():
                        times[name].append(timed(leg, a.iters, a.warmup))
                r = {"S": S, "T": 3 * L, "K": K, "N": N, "beam": beam, "entries_listed": int(nb.nbest_count.sum()),
                     "tokens_per_entry": round(float(nb.hyp_len.sum()) / max(1, int(nb.nbest_count.sum())), 1)}
                for name, model, w in (("order5", lang["order5"], None), ("word3", lang["word3"], words)):
                    tot = torch.zeros(8, dtype=torch.float64, device="cuda")
                    k.ctc_nbest_rescore(nb, add=model, sub=lang["bigram"], words=w, totals=tot)
                    t = tot.cpu().tolist()
                    assert t[0] == S
                    r[name] = {"changed_1best": int(t[4]), "first_pass_errors": t[5], "rescored_errors": t[6], "forbidden": int(t[3]),
                               "oov_words": int(t[7])}
                for name, v in times.items():
                    r[name] = round(statistics.median(v), 1)
                    r[name + "_min_max"] = [round(min(v), 1), round(max(v), 1)]
                r["workspace_bytes"] = k.ctc_rescore_workspace_bytes(S, N, min(1023, 3 * L))
                rows.append(r)
                print(json.dumps(r), flush=True)
    out = {"what": "device microseconds per call through the Python entries, median of %d trials of %d calls; K = 32, words of 4 tokens, "
                   "a token bigram fused into the search and taken out by every second pass" % (TRIALS, a.iters),
           "models": {n: {"states": lang[n].states, "arcs": lang[n].arcs, "classes": lang[n].classes} for n in ("bigram", "order5", "word3")},
           "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
