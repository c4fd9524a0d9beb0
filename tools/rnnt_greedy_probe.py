"""What greedy transducer decoding costs (include/klstm_rnnt.h): device time at S = 8, T = 500, J = 512, V in {64, 1024} of
  * krnnt_greedy_begin + the first krnnt_greedy_step (every chunk of every stream is scanned: the dearest step),
  * a whole decode through rnnt_greedy_decode with a stand-in predictor (a label embedding: one small product per step, no state) and
    the default poll_every = 8: the live count is read back every eighth step and the loop ends when it is 0,
  * for orientation only, the frame-synchronous loop written in torch on the same inputs (one joint row per stream and step, T + MAX_LEN
    steps, nothing read back).
The blank's bias is set so that a stream emits about 50 labels (the offsets were found on the CPU; the counts are recorded).  Device
events around warmed-up repeats that end in a synchronise, the legs alternating, TRIALS times; the median and the spread are kept.
Writes profiles/rnnt_greedy_probe.json.

    python tools/rnnt_greedy_probe.py [--iters 3] [--warmup 1] [--out profiles/rnnt_greedy_probe.json]"""
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

TRIALS = 5
S, T, J, MAX_SYMBOLS, MAX_LEN = 8, 500, 512, 3, 160
BLANK_OFFSET = {64: 2.65, 1024: 3.55}


def inputs(V, device):
    """seeded on the CPU, so that the offsets above can be found without a GPU"""
    g = torch.Generator().manual_seed(V)
    enc, E = torch.randn(T * S, J, generator=g), torch.randn(V, J, generator=g)
    W, b = (torch.rand(V, J, generator=g) - 0.5) * 0.2, torch.zeros(V)
    b[0] = BLANK_OFFSET[V]
    return [x.to(device) for x in (enc, E, W, b)]


def frame_synchronous(enc, E, W, b, steps):
    """plain greedy, all streams side by side, one node per stream and step; returns the labels emitted per stream"""
    dev = enc.device
    e3, ar = enc.view(T, S, J), torch.arange(S, device=dev)
    t, n, count = (torch.zeros(S, dtype=torch.long, device=dev) for _ in range(3))
    p = E[-1].expand(S, J).clone()                          # bos: the last class
    for _ in range(steps):
        live = t < T
        a = torch.tanh(e3[t.clamp(max=T - 1), ar] + p) @ W.T + b
        lab = a.argmax(1)
        emit = live & (lab != 0)
        p = torch.where(emit[:, None], E[lab], p)
        n = torch.where(emit, n + 1, torch.zeros_like(n))
        move = live & (~emit | (n >= MAX_SYMBOLS))
        t, n, count = t + move, torch.where(move, torch.zeros_like(n), n), count + emit
    return count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnnt_greedy_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    res = {"S": S, "T": T, "J": J, "max_symbols": MAX_SYMBOLS, "max_len": MAX_LEN, "shapes": {}}
    for V in (64, 1024):
        enc, E, W, b = inputs(V, "cuda")
        lens = torch.full((S,), T, dtype=torch.int32, device="cuda")
        predictor = lambda next_in: next_in @ E
        state = torch.empty(k.rnnt_greedy_state_bytes(T, S, J), dtype=torch.uint8, device="cuda")
        ints = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")
        next_in, out = torch.empty(S, V, device="cuda"), dict(hyp=ints(S, MAX_LEN), hyp_len=ints(S), frames=ints(S, MAX_LEN),
                                                              score=torch.zeros(S, device="cuda"), flags=ints(S), live=ints(1))
        rows = predictor(torch.nn.functional.one_hot(torch.full((S,), V - 1), V).float().cuda())

        def first_step():
            k.rnnt_greedy_begin(T, S, J, V, V - 1, lens, next_in, state)
            k.rnnt_greedy_step(enc, rows, W, b, T, S, 0, MAX_SYMBOLS, next_in, state=state, **out)

        decode = lambda: k.rnnt_greedy_decode(enc, lens, W, b, predictor, V - 1, blank=0, max_symbols=MAX_SYMBOLS, max_len=MAX_LEN)
        got, want = decode(), frame_synchronous(enc, E, W, b, T + MAX_LEN).tolist()
        labels = [len(y) for y in got["tokens"]]
        legs = {"begin_and_first_step": first_step, "whole_decode": decode, "torch_frame_synchronous": lambda: frame_synchronous(enc, E, W, b, T + MAX_LEN)}
        times = {name: [] for name in legs}
        for _ in range(TRIALS):
            for name, leg in legs.items():
                times[name].append(timed(leg, a.iters, a.warmup))
        shape = {"labels_per_stream": labels, "labels_per_stream_torch_loop": want, "steps": got["steps"], "flags": got["flags"].tolist(), "legs": {}}
        for name, v in times.items():
            us = statistics.median(v)
            shape["legs"][name] = {"us": round(us, 1), "us_min_max": [round(min(v), 1), round(max(v), 1)]}
            print("V %-5d %-26s %10.1f us  (%.1f .. %.1f)" % (V, name, us, min(v), max(v)), flush=True)
        shape["us_per_step_of_whole_decode"] = round(shape["legs"]["whole_decode"]["us"] / got["steps"], 1)
        print("V %-5d labels %s (torch loop %s), %d steps" % (V, labels, want, got["steps"]), flush=True)
        res["shapes"]["V%d" % V] = shape
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"what": "device microseconds per call through the Python entries, median of %d trials of %d calls" % (TRIALS, a.iters), "result": res}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
