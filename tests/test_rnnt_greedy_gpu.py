"""Greedy transducer decoding on the GPU (the krnnt_greedy_* entries of include/klstm_rnnt.h) against the plain
frame-synchronous loop of tests/rnnt_greedy_ref.py, and the C++ layer (TransducerGreedy, DecodeTransducerWholeUtterances of
include/klstm_nnet.hpp) through tests/cpp/rnnt_greedy_test.cpp.

Tokens, frames and flags must EQUAL the float64 truth.  That is meaningful only when no decision on the path is a near-tie, so every case
asserts on the truth alone (a condition on the inputs, not a measurement; the seeds in the table were picked on the CPU to meet it):
the smallest gap between the best and the second-best logit over the path's nodes is >= GAP = 1e-3, and GAP >= 50 x 3e-7 x
max_v sum_j |W_vj| (3e-7: the tanh bound of klstm_math.h, carried through one row of W).  The score's bar is max(4 x the float32 twin's
error, 2^-22) relative, the pair of tests/test_rnnt_gpu.py; the measured figures are in profiles/rnnt_greedy_margins.json.  The shapes
sit at the edges of the scan kernel: chunks of 64 frames (32 for J > 512), 128 classes per register pass, 16 per class tile."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

from tests import cpp_driver
from tests import rnnt_greedy_ref as ref
from tests.margins import bound
from tests.test_rnnt_gpu import FLOOR, MARGIN, SENTINEL, bits, f32, padding_intact, placed

pytestmark = pytest.mark.gpu
GAP = 1e-3
# (T, V, J, S, blank is V - 1, max_symbols, max_len, offset of the blank's bias, seed); S = 3: lengths T, 0 (idle), T - 3
CASES = [(1, 2, 16, 1, 0, 2, 8, -0.5, 1), (63, 17, 16, 1, 1, 3, 200, 1.0, 0), (64, 17, 48, 3, 0, 3, 200, 1.0, 0),
         (65, 129, 16, 1, 0, 3, 200, 1.0, 0), (130, 130, 16, 3, 1, 2, 300, 1.5, 9), (70, 5, 528, 3, 0, 3, 200, 1.5, 0),
         (65, 17, 16, 1, 0, 3, 50, 50.0, 0),                                            # the blank always wins: nothing is emitted
         (20, 17, 16, 1, 0, 1, 100, -50.0, 1), (20, 17, 16, 3, 1, 2, 100, -50.0, 0),    # never: max_symbols moves every frame on
         (64, 17, 16, 1, 0, 3, 5, 0.5, 0)]                                              # max_len truncates
RAGGED = (64, 17, 48, 3, 0, 3, 200, 1.0, 0)
ids = lambda c: "T%d-V%d-J%d-S%d-b%d-m%d-L%d-o%g-s%d" % c


@functools.lru_cache(maxsize=None)
def problem(T, V, J, S, blank_last, max_symbols, max_len, offset, seed):
    rng = np.random.RandomState(seed + 11 * T + V)
    blank, bos = (V - 1, 0) if blank_last else (0, V - 1)
    enc, table = rng.randn(T * S, J).astype(f32), rng.randn(V, J)
    W, b = rng.uniform(-1, 1, (V, J)).astype(f32) * f32(min(0.3, 100.0 / J)), rng.uniform(-0.3, 0.3, V).astype(f32)
    b[blank] += offset
    lens = [T, 0, max(T - 3, 1)] if S == 3 else [T] * S
    pred_fn = ref.history_rows(table)
    truth, twin = [ref.greedy(enc, pred_fn, W, b, lens, blank, bos, max_symbols, max_len, dt) for dt in (torch.float64, torch.float32)]
    return dict(enc=enc, W=W, b=b, lens=lens, blank=blank, bos=bos, pred_fn=pred_fn, truth=truth, twin=twin)


class HistoryPredictor:
    """the predictor of the kernel tests on the device side: reads the label out of each one-hot row, returns pred_fn's float32 rows"""
    def __init__(self, pred_fn, S, J):
        self.pred_fn, self.J, self.history = pred_fn, J, [[] for _ in range(S)]

    def __call__(self, next_in):
        x = next_in.cpu().numpy()
        rows = np.zeros((len(self.history), self.J), f32)
        for s, h in enumerate(self.history):
            if x[s].any():
                h.append(int(x[s].argmax()))
                rows[s] = self.pred_fn(s, h)
        return torch.from_numpy(rows).cuda()


def decode(p, case, order=None, **kw):
    import kaldi_lstm_amd as k
    T, V, J, S = case[:4]
    order = list(range(S)) if order is None else order
    enc = torch.from_numpy(np.ascontiguousarray(p["enc"].reshape(T, S, J)[:, order].reshape(-1, J))).cuda()
    pred = HistoryPredictor(lambda i, h: p["pred_fn"](order[i], h), len(order), J)
    res = k.rnnt_greedy_decode(enc, [p["lens"][s] for s in order], torch.from_numpy(p["W"]).cuda(), torch.from_numpy(p["b"]).cuda(), pred,
                               p["bos"], blank=p["blank"], max_symbols=case[5], max_len=case[6], **kw)
    return dict(res, score=res["score"].cpu().numpy(), flags=res["flags"].tolist())


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_tokens_frames_and_score_against_float64(case):
    p = problem(*case)
    assert GAP >= 50 * 3e-7 * float(np.abs(p["W"]).sum(1).max()), "the condition on W"
    assert all(t["gap"] >= GAP for t in p["truth"]), "a near-tie on the path: %s" % [t["gap"] for t in p["truth"]]
    res = decode(p, case)
    figures = []
    for s, (truth, twin) in enumerate(zip(p["truth"], p["twin"])):
        assert (res["tokens"][s], res["frames"][s], res["flags"][s]) == (truth["tokens"], truth["frames"], truth["flags"]), s
        scale = max(abs(truth["score"]), 1e-300)
        figures.append((abs(float(res["score"][s]) - truth["score"]) / scale, max(MARGIN * abs(twin["score"] - truth["score"]) / scale, FLOOR)))
        print("MARGIN", json.dumps(dict(case=ids(case), stream=s, labels=len(truth["tokens"]), score=truth["score"], err=figures[-1][0],
                                        bar=figures[-1][1])), flush=True)
    for s, (err, bar) in enumerate(figures):
        bound(err, bar, "score of stream %d" % s)


def test_runs_and_stream_company_leave_the_bits_alone():
    p = problem(*RAGGED)
    one, two = decode(p, RAGGED), decode(p, RAGGED, poll_every=1)
    assert one["tokens"] == two["tokens"] and one["frames"] == two["frames"] and np.array_equal(bits(one["score"]), bits(two["score"]))
    assert len(one["tokens"][0]) > 2 and len(one["tokens"][2]) > 2
    for order in ([0], [1], [2], [2, 0, 1], [1, 2, 0]):
        sub = decode(p, RAGGED, order)
        for i, s in enumerate(order):
            assert (sub["tokens"][i], sub["frames"][i], sub["flags"][i]) == (one["tokens"][s], one["frames"][s], one["flags"][s]), (order, s)
            assert bits(sub["score"])[i] == bits(one["score"])[s], (order, s)


def test_steps_after_the_end_change_nothing():
    """the thin wrappers on padded enc and next_in buffers: three more steps after the last stream has stopped"""
    import kaldi_lstm_amd as k
    case = RAGGED
    T, V, J, S, _, max_symbols, max_len = case[:7]
    p = problem(*case)
    (enc, enc_buf), (next_in, next_buf) = placed(p["enc"], 1), placed(np.zeros((S, V), f32), 1)
    W, b, lens = torch.from_numpy(p["W"]).cuda(), torch.from_numpy(p["b"]).cuda(), torch.tensor(p["lens"], dtype=torch.int32, device="cuda")
    ints = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device="cuda")
    out = dict(hyp=ints(S, max_len), hyp_len=ints(S), frames=ints(S, max_len), score=torch.zeros(S, device="cuda"), flags=ints(S), live=ints(1))
    state = torch.zeros(k.rnnt_greedy_state_bytes(T, S, J), dtype=torch.uint8, device="cuda")
    pred = HistoryPredictor(p["pred_fn"], S, J)
    k.rnnt_greedy_begin(T, S, J, V, p["bos"], lens, next_in, state)
    snaps, after = [], None
    for _ in range(max_len + 4):
        k.rnnt_greedy_step(enc, pred(next_in), W, b, T, S, p["blank"], max_symbols, next_in, state=state, **out)
        if after is not None or int(out["live"]) == 0:
            snaps.append({name: t.cpu().numpy().copy() for name, t in out.items()})
            after = len(snaps)
            if after == 4:
                break
    assert after == 4 and all(np.array_equal(snaps[0][name].view(np.uint32), s[name].view(np.uint32)) for s in snaps[1:] for name in out)
    n = snaps[0]["hyp_len"]
    assert [snaps[0]["hyp"][s, :n[s]].tolist() for s in range(S)] == [t["tokens"] for t in p["truth"]]
    assert not next_in.any() and padding_intact(next_in, next_buf, 1) and padding_intact(enc, enc_buf, 1)


# (what is wrong, the status of krnnt_greedy_begin, the status of krnnt_greedy_step; None: the entry does not see it and is not called)
BAD = [("T_s above T", 0, 0), ("T_s negative", 0, 0), ("S", 2, 2), ("T", 2, 2), ("J", 2, 2), ("V", 2, 2), ("bos", 2, None), ("blank", 0, 2),
       ("max_len", 0, 2), ("max_symbols", 0, 2), ("null enc", 0, 1), ("null hyp", 0, 1), ("enc stride", 0, 1), ("misaligned enc", 0, 1),
       ("next_in stride", 1, 1), ("short state", 1, 1), ("misaligned state", 1, 1)]


@pytest.mark.parametrize("how,begin_status,step_status", BAD, ids=[c[0].replace(" ", "_") for c in BAD])
def test_rejection_limits_and_argument_errors(how, begin_status, step_status):
    import kaldi_lstm_amd as k
    lib = k.load_library()
    T, S, J, V, max_len = 5, 2, 16, 5, 4
    x = lambda *shape: torch.full(shape, SENTINEL, device="cuda")
    ints = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device="cuda")
    rng = np.random.RandomState(2)
    enc, pred = torch.from_numpy(rng.randn(T * S, J).astype(f32)).cuda(), torch.from_numpy(rng.randn(S, J).astype(f32)).cuda()
    W, b, next_in = torch.from_numpy(rng.uniform(-0.3, 0.3, (V, J)).astype(f32)).cuda(), torch.zeros(V, device="cuda"), x(S, V)
    lens = torch.tensor([T, {"T_s above T": T + 1, "T_s negative": -1}.get(how, T)], dtype=torch.int32, device="cuda")
    hyp, hyp_len, frames, score, flags, live = ints(S, max_len), ints(S), ints(S, max_len), x(S), ints(S), ints(1)
    nbytes = k.rnnt_greedy_state_bytes(T, S, J)
    state = torch.zeros(nbytes + 256, dtype=torch.uint8, device="cuda")
    a = dict(T=T, S=S, J=J, V=V, bos=V - 1, blank=0, max_symbols=2, max_len=max_len, enc=enc.data_ptr(), es=J, hyp=hyp.data_ptr(), ns=V,
             state=state.data_ptr(), nbytes=nbytes)
    a.update({"S": dict(S=33), "T": dict(T=0), "J": dict(J=24), "V": dict(V=4097), "blank": dict(blank=V), "bos": dict(bos=-1),
              "max_len": dict(max_len=1024), "max_symbols": dict(max_symbols=0), "null enc": dict(enc=None), "null hyp": dict(hyp=None),
              "enc stride": dict(es=J - 1), "next_in stride": dict(ns=V - 1), "short state": dict(nbytes=nbytes - 1),
              "misaligned state": dict(state=state.data_ptr() + 4), "misaligned enc": dict(enc=enc.data_ptr() + 2)}.get(how, {}))
    assert lib.krnnt_greedy_begin(a["T"], a["S"], a["J"], a["V"], a["bos"], lens.data_ptr(), None, None, 0, next_in.data_ptr(), a["ns"],
                                  a["state"], ctypes.c_size_t(a["nbytes"]), None) == begin_status
    if step_status is not None:
        assert lib.krnnt_greedy_step(a["enc"], a["es"], pred.data_ptr(), J, W.data_ptr(), b.data_ptr(), a["T"], a["S"], a["J"], a["V"], a["blank"],
                                     a["max_symbols"], a["max_len"], None, None, 0, next_in.data_ptr(), a["ns"], a["hyp"], hyp_len.data_ptr(),
                                     frames.data_ptr(), score.data_ptr(), flags.data_ptr(), live.data_ptr(), a["state"],
                                     ctypes.c_size_t(a["nbytes"]), None) == step_status
    torch.cuda.synchronize()
    if begin_status:
        assert bool((next_in == SENTINEL).all()) and not state.any()
    if step_status != 0:
        assert all(bool((t == -7).all()) for t in (hyp, hyp_len, frames, flags, live)) and bool((score == SENTINEL).all())
    else:                                                # stream 1 is rejected on the device: no labels, score 0, a zero input row; stream 0 runs
        assert flags.tolist()[1] == ref.REJECTED and hyp_len.tolist()[1] == 0 and float(score[1]) == 0.0 and bool((hyp[1] == -7).all())
        assert flags.tolist()[0] in (0, ref.FINISHED) and not next_in[1].any() and int(live) == (flags.tolist()[0] == 0)


def test_cpp_decoder_is_the_plain_greedy_loop(tmp_path):
    """tests/cpp/rnnt_greedy_test.cpp decodes three utterances with the small model of rnnt_test.cpp (LSTM predictor behind an embedding
    Affine), two streams, with poll_every = 1 and 0, and writes enc, W, b, the hypotheses and the predictor's teacher-forced rows over
    each hypothesis.  The float64 loop over those rows (pred_fn: a row lookup) must reproduce tokens and frames under the gap condition;
    three utterances on two streams leave one stream idle in the last batch."""
    path = str(tmp_path / "dump.json")
    head = cpp_driver.run("rnnt_greedy_test", path).stdout.split()
    d = json.load(open(path))
    assert head[:2] == ["OK", "1"], "poll_every = 1 and 0 disagree"
    W, b = np.asarray(d["W"], f32).reshape(d["V"], d["J"]), np.asarray(d["b"], f32)
    assert GAP >= 50 * 3e-7 * float(np.abs(W).sum(1).max())
    assert len(d["utts"]) == 3 and sum(len(u["tokens"]) for u in d["utts"]) == d["labels"] > 3
    for u in d["utts"]:
        enc, rows = np.asarray(u["enc"], f32).reshape(-1, d["J"]), np.asarray(u["pred"], f32).reshape(-1, d["J"])
        assert len(rows) == len(u["tokens"]) + 1
        truth = ref.greedy(enc, lambda s, h: rows[len(h) - 1], W, b, [len(enc)], d["blank"], d["bos"], d["max_symbols"], d["max_len"], torch.float64)[0]
        assert truth["gap"] >= GAP, truth["gap"]
        assert (u["tokens"], u["frames"], u["flags"]) == (truth["tokens"], truth["frames"], truth["flags"])
