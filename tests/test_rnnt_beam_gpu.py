"""Transducer beam search on the GPU (the krnnt_beam_* entries of include/klstm_rnnt.h) against the plain search of
tests/rnnt_beam_ref.py, against brute force, and against krnnt_eval; krnnt_gather_state, which reorders the predictor's state; and the
C++ layer (TransducerBeam, DecodeTransducerBeamWholeUtterances of include/klstm_nnet.hpp) through tests/cpp/rnnt_beam_test.cpp.

Tokens, counts, flags and the parents of every step must EQUAL the float64 truth.  That is meaningful only when no deciding comparison is
a near-tie, so every case asserts on the truth alone (the seeds were picked on the CPU to meet it): the smallest margin the yardstick
met is >= GAP = 1e-3, and GAP >= 50 x 3e-7 x max_v sum_j |W_vj| (the pair of tests/test_rnnt_greedy_gpu.py).  The score's bar is
max(4 x the float32 twin's error, 2^-22) relative; the measured figures are in profiles/rnnt_beam_margins.json.  The shapes sit at the
edges of the scan kernel: chunks of 64 frames (32 for J > 512), one sweep up to 128 classes and two above, 16 classes per tile."""
import ctypes
import functools
import json
import math

import numpy as np
import pytest
import torch

from tests import cpp_driver, rnnt_beam_ref as ref
from tests.margins import bound
from tests.rnnt_greedy_ref import history_rows
from tests.test_rnnt_gpu import FLOOR, MARGIN, SENTINEL, bits, f32

pytestmark = pytest.mark.gpu
GAP = 1e-3
# (T, V, J, S, B, N, max_len, offset of the blank's bias (None: log((V - 1) T / 8), a few labels per utterance), seed); S = 3: lengths
# T, 0 (idle), T + 1 (rejected); S = 4: T, 0, T - 3, T + 1
CASES = [(1, 2, 16, 1, 1, 1, 8, 0.0, 0), (63, 17, 16, 1, 2, 2, 40, None, 0), (64, 128, 48, 3, 4, 2, 40, None, 0),
         (65, 129, 16, 1, 2, 1, 40, None, 0), (130, 130, 16, 4, 4, 4, 40, None, 7), (66, 5, 528, 3, 2, 2, 40, None, 0),
         (65, 5, 512, 1, 2, 2, 40, None, 0),                                            # the widest joint that keeps chunks of 64 frames
         (65, 17, 16, 1, 2, 1, 40, 50.0, 0),                                            # the blank always wins: the empty list entry
         (20, 17, 16, 1, 2, 2, 3, -50.0, 0)]                                            # never: the search runs into max_len
EXACT = [(1, 3, 16, 1, 16, 4, 4, 0.5, 0), (5, 3, 16, 1, 16, 4, 4, 1.0, 0), (5, 4, 16, 1, 32, 8, 3, 1.5, 1)]
RAGGED = CASES[4]
ids = lambda c: "T%d-V%d-J%d-S%d-B%d-N%d-L%d-o%s-s%d" % c


@functools.lru_cache(maxsize=None)
def problem(T, V, J, S, B, N, max_len, offset, seed):
    rng = np.random.RandomState(seed + 11 * T + V)
    blank, bos = 0, V - 1
    enc, table = rng.randn(T * S, J).astype(f32), rng.randn(V, J)
    W, b = rng.uniform(-1, 1, (V, J)).astype(f32) * f32(min(0.3, 100.0 / J)), rng.uniform(-0.3, 0.3, V).astype(f32)
    b[blank] += math.log((V - 1) * T / 8.0) if offset is None else offset
    lens = {3: [T, 0, T + 1], 4: [T, 0, T - 3, T + 1]}.get(S, [T] * S)
    pred_fn = history_rows(table)
    truth, twin = [ref.beam(enc, pred_fn, W, b, lens, blank, bos, B, N, max_len, dt) for dt in (torch.float64, torch.float32)]
    return dict(enc=enc, W=W, b=b, lens=lens, blank=blank, bos=bos, table=table, pred_fn=pred_fn, truth=truth, twin=twin)


def decode(p, case, order=None, **kw):
    """the search on the GPU with the stand-in predictor p_u = table[x_u] + 0.5 p_{u-1}, whose state follows the parents; returns the
    lists, the flags and per step and stream the (parent slot, label) of every new slot"""
    import kaldi_lstm_amd as k
    T, V, J, S, B, N, max_len = case[:7]
    order = list(range(S)) if order is None else order
    state, steps = [np.zeros((len(order) * B, J))], []

    def pred_fn(next_in, parents):
        x, par = next_in.cpu().numpy(), parents.cpu().numpy()
        new = np.zeros_like(state[0])
        for i in np.flatnonzero(x.any(1)):
            new[i] = p["table"][x[i].argmax()] + 0.5 * (state[0][par[i]] if par[i] >= 0 else 0.0)
        steps.append([[(int(par[i]) - s * B, int(x[i].argmax())) for i in range(s * B, s * B + B) if x[i].any()] for s in range(len(order))])
        state[0] = new
        return torch.from_numpy(new.astype(f32)).cuda()

    enc = torch.from_numpy(np.ascontiguousarray(p["enc"].reshape(T, S, J)[:, order].reshape(-1, J))).cuda()
    res = k.rnnt_beam_decode(enc, [p["lens"][s] for s in order], pred_fn, torch.from_numpy(p["W"]).cuda(), torch.from_numpy(p["b"]).cuda(),
                             p["bos"], blank=p["blank"], beam=B, nbest=N, max_len=max_len, **kw)
    return dict(res, score=res["score"].cpu().numpy(), flags=res["flags"].tolist(), steps=steps[1:])


def check(case, p, res, s, truth, twin):
    assert GAP >= 50 * 3e-7 * float(np.abs(p["W"]).sum(1).max()), "the condition on W"
    assert truth["gap"] >= GAP, "a near-tie decides: %g" % truth["gap"]
    assert ([y for y, _ in res["nbest"][s]], res["flags"][s]) == ([y for y, _ in truth["nbest"]], truth["flags"]), s
    for u, want in enumerate(truth["steps"]):                        # (the selection of the last step is never fed to the predictor)
        assert (res["steps"][u][s] if u < len(res["steps"]) else []) == want, (s, u)
    assert all(not st[s] for st in res["steps"][len(truth["steps"]):])
    for q, (y, sc) in enumerate(truth["nbest"]):
        tw = twin["nbest"][q][1] if q < len(twin["nbest"]) and twin["nbest"][q][0] == y else sc
        err, bar = abs(res["nbest"][s][q][1] - sc) / max(abs(sc), 1e-300), max(MARGIN * abs(tw - sc) / max(abs(sc), 1e-300), FLOOR)
        print("MARGIN", json.dumps(dict(case=ids(case), stream=s, rank=q, labels=len(y), score=sc, err=err, bar=bar)), flush=True)
        bound(err, bar, "score %d of stream %d" % (q, s))


@pytest.mark.parametrize("case", EXACT, ids=ids)
def test_unpruned_search_is_brute_force(case):
    p = problem(*case)
    best, gap = ref.brute_force(p["enc"], p["pred_fn"], p["W"], p["b"], p["blank"], p["bos"], case[6], case[5])
    assert gap >= GAP, gap
    assert [y for y, _ in p["truth"][0]["nbest"]] == [y for y, _ in best] and not p["truth"][0]["flags"] & ref.PRUNED
    assert max(abs(a[1] - c[1]) for a, c in zip(p["truth"][0]["nbest"], best)) < 1e-9
    check(case, p, decode(p, case), 0, p["truth"][0], p["twin"][0])


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_pruned_search_against_float64(case):
    p = problem(*case)
    res = decode(p, case)
    for s, (truth, twin) in enumerate(zip(p["truth"], p["twin"])):
        check(case, p, res, s, truth, twin)
    flags = [t["flags"] for t in p["truth"]]
    assert flags[0] & (ref.TRUNCATED if case[7] == -50.0 else ref.FINISHED) and (case[3] == 1 or (flags[1], flags[-1]) == (ref.IDLE, ref.REJECTED))
    assert case[7] != 50.0 or res["nbest"][0] == [([], res["nbest"][0][0][1])] and res["steps"][0] == [[]]


@pytest.mark.parametrize("case", [CASES[1], CASES[3]], ids=ids)
def test_scores_are_those_of_training(case):
    """every listed hypothesis as a stream of a forward-only krnnt_eval: the same number within the bar"""
    import kaldi_lstm_amd as k
    p = problem(*case)
    hyps = decode(p, case)["nbest"][0]
    ys, Umax = [y for y, _ in hyps], max(len(y) for y, _ in hyps)
    pred = np.zeros(((Umax + 1), len(ys), case[2]), f32)
    for i, y in enumerate(ys):
        for u in range(len(y) + 1):
            pred[u, i] = p["pred_fn"](0, [p["bos"]] + y[:u])
    enc = torch.from_numpy(np.repeat(p["enc"], len(ys), 0)).cuda()
    loss = k.rnnt_eval(enc, torch.from_numpy(pred.reshape(-1, case[2])).cuda(), torch.from_numpy(p["W"]).cuda(), torch.from_numpy(p["b"]).cuda(),
                       [case[0]] * len(ys), ys, blank=p["blank"], want_grads=False)["loss"].cpu().numpy()
    for q, ((y, sc), (_, truth), (_, twin)) in enumerate(zip(hyps, p["truth"][0]["nbest"], p["twin"][0]["nbest"])):
        bound(abs(sc + float(loss[q])) / abs(truth), max(MARGIN * abs(twin - truth) / abs(truth), FLOOR), "score %d against krnnt_eval" % q)


def test_runs_and_stream_company_leave_the_bits_alone():
    p = problem(*RAGGED)
    one, two = decode(p, RAGGED), decode(p, RAGGED, poll_every=1)
    assert one["nbest"] == two["nbest"] and np.array_equal(bits(one["score"]), bits(two["score"])) and one["steps"][:len(two["steps"])] == two["steps"]
    assert len(one["nbest"][0]) > 1 and len(one["nbest"][2]) > 1 and one["steps"] > two["steps"]      # steps after the end change nothing
    for order in ([0], [1], [2], [3, 2, 0, 1], [1, 2, 0]):
        sub = decode(p, RAGGED, order)
        for i, s in enumerate(order):
            assert sub["nbest"][i] == one["nbest"][s] and sub["flags"][i] == one["flags"][s], (order, s)
            assert np.array_equal(bits(sub["score"])[i], bits(one["score"])[s]), (order, s)


# (what is wrong, the status of krnnt_beam_begin, the status of krnnt_beam_step; None: the entry does not see it and is not called)
BAD = [("T_s above T", 0, 0), ("S", 2, 2), ("B", 2, 2), ("T", 2, 2), ("J", 2, 2), ("V", 2, 2), ("bos", 2, None), ("blank", 0, 2), ("N above B", 0, 2),
       ("max_len", 0, 2), ("null enc", 0, 1), ("null hyp", 0, 1), ("enc stride", 0, 1), ("misaligned enc", 0, 1), ("next_in stride", 1, 1),
       ("short state", 1, 1), ("misaligned state", 1, 1)]


@pytest.mark.parametrize("how,begin_status,step_status", BAD, ids=[c[0].replace(" ", "_") for c in BAD])
def test_rejection_limits_and_argument_errors(how, begin_status, step_status):
    import kaldi_lstm_amd as k
    lib = k.load_library()
    T, S, B, N, J, V, max_len = 5, 2, 2, 2, 16, 5, 4
    x = lambda *shape: torch.full(shape, SENTINEL, device="cuda")
    ints = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device="cuda")
    rng = np.random.RandomState(2)
    enc, pred = torch.from_numpy(rng.randn(T * S, J).astype(f32)).cuda(), torch.from_numpy(rng.randn(S * B, J).astype(f32)).cuda()
    W, b, next_in = torch.from_numpy(rng.uniform(-0.3, 0.3, (V, J)).astype(f32)).cuda(), torch.zeros(V, device="cuda"), x(S * B, V)
    lens = torch.tensor([T, T + 1 if how == "T_s above T" else T], dtype=torch.int32, device="cuda")
    parents, hyp, hyp_len, score, count, flags, live = ints(S * B), ints(S, N, max_len), ints(S, N), x(S, N), ints(S), ints(S), ints(1)
    nbytes = k.rnnt_beam_state_bytes(T, S, B, J, V)
    up, SB, nc = lambda n: (n + 255) // 256 * 256, S * B, 1                # the header's formula, term by term
    assert nbytes == (5 * up(4 * S) + up(256 * S) + up(128 * S) + 3 * up(4 * SB) + up(8192 * SB) + 3 * up(8 * SB * T) + 2 * up(4 * SB * T) +
                      4 * up(8 * SB * nc) + up(8 * V * SB * nc) + up(8 * SB * V))
    state = torch.zeros(nbytes + 256, dtype=torch.uint8, device="cuda")
    a = dict(T=T, S=S, B=B, N=N, J=J, V=V, bos=V - 1, blank=0, max_len=max_len, enc=enc.data_ptr(), es=J, hyp=hyp.data_ptr(), ns=V,
             state=state.data_ptr(), nbytes=nbytes)
    a.update({"S": dict(S=33), "B": dict(B=33), "T": dict(T=0), "J": dict(J=24), "V": dict(V=4097), "blank": dict(blank=V), "bos": dict(bos=-1),
              "N above B": dict(N=B + 1), "max_len": dict(max_len=1024), "null enc": dict(enc=None), "null hyp": dict(hyp=None),
              "enc stride": dict(es=J - 1), "next_in stride": dict(ns=V - 1), "short state": dict(nbytes=nbytes - 1),
              "misaligned state": dict(state=state.data_ptr() + 4), "misaligned enc": dict(enc=enc.data_ptr() + 2)}.get(how, {}))
    assert lib.krnnt_beam_begin(a["T"], a["S"], a["B"], a["J"], a["V"], a["bos"], lens.data_ptr(), None, None, 0, next_in.data_ptr(), a["ns"],
                                parents.data_ptr(), a["state"], ctypes.c_size_t(a["nbytes"]), None) == begin_status
    if step_status is not None:
        assert lib.krnnt_beam_step(a["enc"], a["es"], pred.data_ptr(), J, W.data_ptr(), b.data_ptr(), a["T"], a["S"], a["B"], a["N"], a["J"], a["V"],
                                   a["blank"], a["max_len"], None, None, 0, next_in.data_ptr(), a["ns"], parents.data_ptr(), a["hyp"],
                                   hyp_len.data_ptr(), score.data_ptr(), count.data_ptr(), flags.data_ptr(), live.data_ptr(), a["state"],
                                   ctypes.c_size_t(a["nbytes"]), None) == step_status
    torch.cuda.synchronize()
    if begin_status:
        assert bool((next_in == SENTINEL).all()) and bool((parents == -7).all()) and not state.any()
    if step_status != 0:
        assert all(bool((t == -7).all()) for t in (hyp, hyp_len, count, flags, live)) and bool((score == SENTINEL).all())
    else:                                                # stream 1 is rejected on the device: an empty list, zero input rows; stream 0 runs
        assert flags.tolist()[1] == ref.REJECTED and count.tolist() == [1, 0] and not next_in[B:].any() and parents.tolist()[B:] == [-1] * B
        assert int(live) == int((parents >= 0).sum()) > 0


def test_gather_state_is_set_state_of_the_gathered_arrays():
    import kaldi_lstm_amd as k
    from oracle.oracle import make_params
    I, C, R, S = 40, 64, 32, 4
    x = [torch.from_numpy(np.random.RandomState(i).randn(2 * S, I).astype(f32)).cuda() for i in range(2)]
    src = [1, 1, 0, -1]                                    # a duplicate, a swap of 0 and 1, no source
    outs = []
    for device_side in (True, False):
        e, out = k.Engine(I, C, R, S, device=0), torch.empty(2 * S, R, device="cuda")
        e.set_params(make_params(I, C, R, scale=0.3, seed=3))
        e.propagate(x[0], out)
        c, r = e.get_state()
        want = [np.where(np.asarray(src)[:, None] >= 0, m[src], 0).astype(f32) for m in (c, r)]
        if device_side:
            e.gather_state(torch.tensor(src, dtype=torch.int32, device="cuda"))
            assert all(np.array_equal(bits(g), bits(w)) for g, w in zip(e.get_state(), want)) and np.abs(want[0][:3]).min() > 0
        else:
            e.set_state(*want)
        e.propagate(x[1], out)
        e.synchronize()
        outs.append(bits(out))
        e.close()
    assert np.array_equal(outs[0], outs[1])


def test_cpp_decoder_is_the_float64_search_over_teacher_forced_rows(tmp_path):
    """tests/cpp/rnnt_beam_test.cpp decodes three utterances on two streams with beam 3 (an LSTM predictor of six streams whose state
    follows the parents through Nnet::GatherStreams), with poll_every = 1 and 0, and writes the predictor's teacher-forced row of every
    label prefix up to max_len.  The float64 search over those rows must give the same lists and flags, the scores within the bar."""
    path = str(tmp_path / "dump.json")
    head = cpp_driver.run("rnnt_beam_test", path).stdout.split()
    d = json.load(open(path))
    assert head[:3] == ["OK", "1", "3"], "poll_every = 1 and 0 disagree, or a predictor of the wrong stream count was accepted"
    W, b = np.asarray(d["W"], f32).reshape(d["V"], d["J"]), np.asarray(d["b"], f32)
    rows = {tuple(q["y"]): np.asarray(q["row"], f32) for q in d["prefixes"]}
    assert GAP >= 50 * 3e-7 * float(np.abs(W).sum(1).max()) and len(rows) == 85 and len(d["utts"]) == 3
    for u in d["utts"]:
        enc = np.asarray(u["enc"], f32).reshape(-1, d["J"])
        truth, twin = [ref.beam(enc, lambda s, h: rows[tuple(h[1:])], W, b, [len(enc)], d["blank"], d["bos"], d["beam"], d["nbest"], d["max_len"], dt)[0]
                       for dt in (torch.float64, torch.float32)]
        assert truth["gap"] >= GAP, truth["gap"]
        assert ([q["tokens"] for q in u["nbest"]], u["flags"]) == ([y for y, _ in truth["nbest"]], truth["flags"]) and len(u["nbest"]) == d["nbest"]
        for q, (_, sc), (_, tw) in zip(u["nbest"], truth["nbest"], twin["nbest"]):
            bound(abs(q["score"] - sc) / abs(sc), max(MARGIN * abs(tw - sc) / abs(sc), FLOOR), "score of %s" % q["tokens"])
