"""What MMI (CTC-CRF) training costs per minibatch: device time of klstm_ctc_mmi_eval (the reference's chains, the denominator's chains
over the language model's graph, the rows of diff) next to klstm_ctc_eval on the same posteriors, and the workspace it needs.  Cells:
T in {200, 1000}, S in {4, 16}, K = 48 with a unigram and a bigram, and a trigram at K = 16; add-k models estimated from the references;
peaked posteriors around references of T / 10 labels (tools/ctc_mbr_probe.py's).  Device events around warmed-up repeats that end in a
synchronise, both legs in the same process.  Prints one JSON line per cell and writes them all to --out (DESIGN.md 4p records them;
profiles/ctc_mmi_probe.json).

    python tools/ctc_mmi_probe.py [--iters 5] [--warmup 2] [--out profiles/ctc_mmi_probe.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kaldi_lstm_amd as k  # noqa: E402
from tools.ctc_mbr_probe import peaked  # noqa: E402
from tools.ctc_probe import timed  # noqa: E402

CELLS = [(order, 48) for order in (1, 2)] + [(3, 16)]


def cell(order, K, S, T, iters, warmup):
    y, lens, refs = peaked(S, T, T // 10, K)
    ld = torch.tensor(lens, dtype=torch.int32, device="cuda")
    packed = k.ctc.pack_labels(refs, y.device)
    lm = k.CtcLabelLm(*k.ngram_label_lm(refs, K, 0, order=order, add_k=0.5))
    den = k.CtcMmiDenominator(lm, blank=0)
    diff = torch.empty_like(y)
    mmi = timed(lambda: k.ctc_mmi_eval(y, ld, packed, den, ctc_weight=0.1, diff=diff), iters, warmup)
    res = k.ctc_mmi_eval(y, ld, packed, den, ctc_weight=0.1, diff=diff)
    ctc = timed(lambda: k.ctc_eval(y, ld, packed, 0, diff), iters, warmup)
    assert bool(torch.isfinite(res.loss).all()) and bool((res.loss >= 0).all())
    return {"order": order, "K": K, "lm_states": lm.states, "S": S, "T": T, "labels": T // 10, "mmi_us": round(mmi, 1), "ctc_us": round(ctc, 1),
            "workspace_mb": round(k.ctc_mmi_workspace_bytes(T, S, K, lm.states, max(len(r) for r in refs)) / 2 ** 20, 1),
            "avg_loss": round(float(res.loss.mean()), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for order, K in CELLS:
        for T in (200, 1000):
            for S in (4, 16):
                rows.append(cell(order, K, S, T, a.iters, a.warmup))
                print(json.dumps(rows[-1]), flush=True)
                torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"command": "python tools/ctc_mmi_probe.py --iters %d --warmup %d" % (a.iters, a.warmup), "device": torch.cuda.get_device_name(0),
                       "cells": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
