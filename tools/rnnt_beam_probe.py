"""What the transducer beam search costs (include/klstm_rnnt.h): device time at the shape of tools/rnnt_greedy_probe.py,
S = 8, T = 500, J = 512, V in {64, 1024}, the same inputs, blank bias and stand-in predictor (a label embedding, no state: the parents
are not needed), beam 4, lists of 4:
  * krnnt_beam_begin + the first krnnt_beam_step,
  * a whole decode through rnnt_beam_decode with the default poll_every = 8, and its time per step,
  * on the same inputs the greedy decode (rnnt_greedy_decode, whose kernels this search leaves as they are) and its time per step: the
    reference point.  The beam step does beam times the greedy step's joint work plus the class reductions; the ratio to beam x greedy
    is recorded, not promised.
Also recorded: the steps, the flags, and for how many streams the 1-best differs from the greedy path.  Device events around warmed-up
repeats that end in a synchronise, the legs alternating, TRIALS times; the median and the spread are kept.
With --margins LOG nothing is measured: the MARGIN lines that `pytest -s tests/test_rnnt_beam_gpu.py` printed into LOG become
profiles/rnnt_beam_margins.json.

    python tools/rnnt_beam_probe.py [--iters 3] [--warmup 1] [--out profiles/rnnt_beam_probe.json]
    python tools/rnnt_beam_probe.py --margins LOG [--out profiles/rnnt_beam_margins.json]"""
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
from tools.rnnt_greedy_probe import J, MAX_LEN, MAX_SYMBOLS, S, T, TRIALS, inputs  # noqa: E402

BEAM, NBEST = 4, 4


def margins(log, out):
    rows = [json.loads(line[line.index("MARGIN ") + 7:]) for line in open(log) if "MARGIN {" in line]
    assert rows, "no MARGIN lines in " + log
    worst = max(rows, key=lambda q: q["err"] / q["bar"])
    with open(out, "w") as fh:
        json.dump({"what": "relative error of every listed score of tests/test_rnnt_beam_gpu.py against the float64 search, and its bar "
                           "max(4 x the float32 twin's error, 2^-22); written by tools/rnnt_beam_probe.py --margins from the test's own output",
                   "tightest_fraction_of_bar": round(worst["err"] / worst["bar"], 4), "tightest": worst, "margins": rows}, fh, indent=1)
        fh.write("\n")
    print("%d margins, the tightest at %.4f of its bar: %s" % (len(rows), worst["err"] / worst["bar"], worst["case"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--margins", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.margins:
        return margins(a.margins, a.out or os.path.join(ROOT, "profiles", "rnnt_beam_margins.json"))
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    res = {"S": S, "T": T, "J": J, "beam": BEAM, "nbest": NBEST, "max_len": MAX_LEN, "greedy_max_symbols": MAX_SYMBOLS, "shapes": {}}
    for V in (64, 1024):
        enc, E, W, b = inputs(V, "cuda")
        lens = torch.full((S,), T, dtype=torch.int32, device="cuda")
        SB = S * BEAM
        state = torch.empty(k.rnnt_beam_state_bytes(T, S, BEAM, J, V), dtype=torch.uint8, device="cuda")
        ints = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")
        next_in, parents = torch.empty(SB, V, device="cuda"), ints(SB)
        out = dict(hyp=ints(S, NBEST, MAX_LEN), hyp_len=ints(S, NBEST), score=torch.zeros(S, NBEST, device="cuda"), count=ints(S), flags=ints(S),
                   live=ints(1))
        rows = torch.zeros(SB, J, device="cuda")
        rows[::BEAM] = E[V - 1]                             # bos in slot 0 of every stream

        def first_step():
            k.rnnt_beam_begin(T, S, BEAM, J, V, V - 1, lens, next_in, parents, state)
            k.rnnt_beam_step(enc, rows, W, b, T, S, BEAM, 0, next_in, parents, state=state, **out)

        beam = lambda: k.rnnt_beam_decode(enc, lens, lambda x, par: x @ E, W, b, V - 1, blank=0, beam=BEAM, nbest=NBEST, max_len=MAX_LEN)
        greedy = lambda: k.rnnt_greedy_decode(enc, lens, W, b, lambda x: x @ E, V - 1, blank=0, max_symbols=MAX_SYMBOLS, max_len=MAX_LEN)
        got, ref = beam(), greedy()
        legs = {"begin_and_first_step": first_step, "whole_decode": beam, "greedy_whole_decode": greedy}
        times = {name: [] for name in legs}
        for _ in range(TRIALS):
            for name, leg in legs.items():
                times[name].append(timed(leg, a.iters, a.warmup))
        best = [lst[0][0] if lst else None for lst in got["nbest"]]
        shape = {"steps": got["steps"], "greedy_steps": ref["steps"], "flags": got["flags"].tolist(), "list_sizes": got["count"].tolist(),
                 "labels_of_1best": [len(y) for y in best], "labels_of_greedy": [len(y) for y in ref["tokens"]],
                 "streams_whose_1best_differs_from_greedy": sum(y != g for y, g in zip(best, ref["tokens"])), "legs": {}}
        for name, v in times.items():
            us = statistics.median(v)
            shape["legs"][name] = {"us": round(us, 1), "us_min_max": [round(min(v), 1), round(max(v), 1)]}
            print("V %-5d %-22s %10.1f us  (%.1f .. %.1f)" % (V, name, us, min(v), max(v)), flush=True)
        per, gper = shape["legs"]["whole_decode"]["us"] / got["steps"], shape["legs"]["greedy_whole_decode"]["us"] / ref["steps"]
        shape.update(us_per_step=round(per, 1), greedy_us_per_step=round(gper, 1), ratio_to_beam_times_greedy_step=round(per / (BEAM * gper), 2))
        print("V %-5d %d steps (greedy %d), %.1f us per step (greedy %.1f): %.2f of beam x greedy; the 1-best differs for %d streams" %
              (V, got["steps"], ref["steps"], per, gper, per / (BEAM * gper), shape["streams_whose_1best_differs_from_greedy"]), flush=True)
        res["shapes"]["V%d" % V] = shape
    with open(a.out or os.path.join(ROOT, "profiles", "rnnt_beam_probe.json"), "w") as fh:
        json.dump({"what": "device microseconds per call through the Python entries, median of %d trials of %d calls" % (TRIALS, a.iters), "result": res}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
