"""The transducer kernels on the GPU (the krnnt_* entries of include/klstm_rnnt.h) against tests/rnnt_ref.py, and the C++ layer over them
(TransducerJoint, Transducer, TrainTransducerWholeUtterances of include/klstm_nnet.hpp) through tests/cpp/rnnt_test.cpp.

Parity: the project's measure, max|gpu - truth64| / max|truth64| per tensor, through margins.bound(); the bar is max(MARGIN x the error of
the float32 twin on the same inputs, FLOOR) with the pair tests/test_cnn_gpu.py uses for exact-f32 products on the matrix instruction:
MARGIN = 4, FLOOR = 2^-22.  No bar comes from the kernels' own output; the measured figures are in profiles/rnnt_parity_margins.json and
DESIGN.md 4x.  The shapes sit at the edges of the tiles (klstm_rnnt.h: 16 t x 8 u per forward tile, 4 u per backward step, 128 classes
per register pass, 16 per class tile; W panels of 32 k and three instances of the backward kernel by J in klstm_rnnt.hip)."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from tests import cpp_driver, rnnt_ref
from tests.margins import bound

pytestmark = pytest.mark.gpu
f32 = np.float32
MARGIN, FLOOR = 4.0, 2.0 ** -22
SENTINEL = 12345.0
TENSORS = ("loss", "d_enc", "d_pred", "W_grad", "b_grad")
# (T, Umax, V, J, S, blank is V - 1, scale of W)
CASES = [(1, 0, 2, 16, 1, 0, 1), (1, 3, 17, 16, 1, 1, 1), (5, 0, 17, 48, 1, 0, 1), (15, 6, 2, 16, 3, 1, 1), (16, 7, 17, 48, 1, 0, 1),
         (17, 8, 129, 48, 3, 1, 1), (33, 16, 130, 16, 3, 0, 1), (17, 9, 17, 48, 3, 0, 8),
         (5, 4, 5, 144, 1, 0, 1), (3, 1, 5, 528, 1, 1, 1)]      # J above 128 and above 512: the other two instances of the backward kernel


def bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=f32).view(np.uint32)


def placed(x, layout):
    """x on the device in a padded buffer: (view, whole buffer); layout: the first column of the view"""
    rows, cols = x.shape
    buf = torch.full((rows, (cols + layout + 1 + 63) // 64 * 64), SENTINEL, device="cuda")
    view = buf[:, layout:layout + cols]
    view.copy_(torch.from_numpy(np.ascontiguousarray(x, dtype=f32)))
    return view, buf


def padding_intact(view, buf, layout):
    b = buf.cpu().numpy().copy()
    b[:, layout:layout + view.shape[1]] = SENTINEL
    return bool((b == SENTINEL).all())


@functools.lru_cache(maxsize=None)
def problem(T, Umax, V, J, S, blank_last, wscale, seed=0):
    """inputs (ragged at S = 3: a repeated label at full length, U = 0, T_s < T) and both references"""
    rng = np.random.RandomState(seed + 7 * T + Umax)
    blank = V - 1 if blank_last else 0
    enc, pred = rng.randn(T * S, J).astype(f32), rng.randn((Umax + 1) * S, J).astype(f32)
    W, b = (wscale * rng.uniform(-0.3, 0.3, (V, J))).astype(f32), rng.uniform(-0.3, 0.3, V).astype(f32)
    lens, ulen = [T] * S, [Umax] * S
    if S == 3:
        lens, ulen = [T, T, max(T - 1, 1)], [Umax, 0, max(Umax - 1, 0)]
    labels = [[int(v) for v in (rng.randint(0, V - 1, n) + (blank == 0))] for n in ulen]
    if Umax >= 2:
        labels[0][1] = labels[0][0]
    refs = [rnnt_ref.transducer(enc, pred, W, b, lens, labels, blank, dt) for dt in (torch.float64, torch.float32)]
    return enc, pred, W, b, lens, labels, blank, refs[0], refs[1]


def run(enc, pred, W, b, lens, labels, blank, **kw):
    import kaldi_lstm_amd as k
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=f32)).cuda()
    return k.rnnt_eval(d(enc) if isinstance(enc, np.ndarray) else enc, d(pred) if isinstance(pred, np.ndarray) else pred, d(W), d(b), lens, labels,
                       blank=blank, **kw)


def check(tag, res, truth, twin):
    figures = []
    for name in TENSORS:
        err, e32 = rnnt_ref.rel_err(res[name].cpu().numpy(), truth[name]), rnnt_ref.rel_err(twin[name], truth[name])
        figures.append((err, max(MARGIN * e32, FLOOR), name))
        print(f"{tag} {name}: {err:.3g} (twin {e32:.3g}, bar {figures[-1][1]:.3g})", flush=True)
    for err, bar, name in figures:
        bound(err, bar, name)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "T%d-U%d-V%d-J%d-S%d-b%d-w%d" % c)
def test_eval_against_float64(case):
    T, Umax, V, J, S = case[:5]
    enc, pred, W, b, lens, labels, blank, truth, twin = problem(*case)
    (ev, eb), (pv, pb) = placed(enc, 0), placed(pred, 1)
    out = {"d_enc": placed(np.full_like(enc, SENTINEL), 1), "d_pred": placed(np.full_like(pred, SENTINEL), 0)}
    totals = torch.zeros(5, dtype=torch.float64, device="cuda")
    res = run(ev, pv, W, b, lens, labels, blank, totals=totals, out={k: v[0] for k, v in out.items()})
    torch.cuda.synchronize()
    assert padding_intact(*out["d_enc"], 1) and padding_intact(*out["d_pred"], 0), "columns outside the rows were written"
    check("%s" % (case,), res, truth, twin)
    want = [truth["loss"].sum(), sum(lens), sum(len(y) for y in labels), S, 0]
    assert np.allclose(totals.cpu().numpy(), want, rtol=1e-5)
    if S == 3:                                           # rows t >= T_s of d_enc and u > U_s of d_pred are written as zero
        assert not res["d_pred"].reshape(Umax + 1, S, J)[1:, 1].any() and (T == 1 or not res["d_enc"].reshape(T, S, J)[T - 1, 2].any())


def test_long_lattice_keeps_its_digits():
    """T = 400, U = 60 (24 k nodes; the reference takes under a second): log alpha reaches -400, where plain fp32 log-domain rows lose
    digits; the same bar holds because of the per-diagonal offsets in double"""
    rng = np.random.RandomState(5)
    T, U, J, V = 400, 60, 16, 4
    enc, pred = rng.randn(T, J).astype(f32), rng.randn(U + 1, J).astype(f32)
    W, b = rng.uniform(-0.3, 0.3, (V, J)).astype(f32), rng.uniform(-0.3, 0.3, V).astype(f32)
    y = [[int(v) for v in rng.randint(1, V, U)]]
    truth, twin = [rnnt_ref.transducer(enc, pred, W, b, [T], y, 0, dt) for dt in (torch.float64, torch.float32)]
    check("long", run(enc, pred, W, b, [T], y, 0), truth, twin)


def test_runs_and_stream_company_leave_the_bits_alone():
    case = (17, 8, 17, 48, 3, 0, 1)
    T, Umax, V, J, S = case[:5]
    enc, pred, W, b, lens, labels, blank = problem(*case)[:7]
    one, two, fwd = [run(enc, pred, W, b, lens, labels, blank, want_grads=g) for g in (True, True, False)]
    for name in TENSORS:
        assert np.array_equal(bits(one[name]), bits(two[name])), f"{name}: two runs differ"
    assert np.array_equal(bits(one["loss"]), bits(fwd["loss"])) and set(fwd) == {"loss"}
    e3, p3 = enc.reshape(T, S, J), pred.reshape(Umax + 1, S, J)
    for order in ([0], [1], [2], [2, 0, 1]):
        sub = run(e3[:, order].reshape(-1, J), p3[:, order].reshape(-1, J), W, b, [lens[s] for s in order], [labels[s] for s in order], blank)
        n = len(order)
        for i, s in enumerate(order):
            assert bits(sub["loss"])[i] == bits(one["loss"])[s]
            assert np.array_equal(bits(sub["d_enc"].view(T, n, J)[:, i]), bits(one["d_enc"].view(T, S, J)[:, s])), (order, s)
            assert np.array_equal(bits(sub["d_pred"].view(Umax + 1, n, J)[:, i]), bits(one["d_pred"].view(Umax + 1, S, J)[:, s])), (order, s)


@pytest.mark.parametrize("how", ["idle", "label out of range", "label equals blank", "U above Umax"])
def test_idle_and_rejected_streams(how):
    T, Umax, V, J, blank = 9, 3, 5, 16, 0
    rng = np.random.RandomState(3)
    enc, pred = rng.randn(T * 2, J).astype(f32), rng.randn((Umax + 1) * 2, J).astype(f32)
    W, b = rng.uniform(-0.3, 0.3, (V, J)).astype(f32), rng.uniform(-0.3, 0.3, V).astype(f32)
    bad = {"idle": [1, 2], "label out of range": [1, V], "label equals blank": [blank, 2], "U above Umax": [1, 2, 3, 4, 1]}[how]
    lens, labels = [T, 0 if how == "idle" else T], [[1, 2, 3], bad]
    alone = run(enc.reshape(T, 2, J)[:, 0], pred.reshape(Umax + 1, 2, J)[:, 0], W, b, [T], [labels[0]], blank)
    out = {"d_enc": torch.full((T * 2, J), SENTINEL, device="cuda"), "d_pred": torch.full(((Umax + 1) * 2, J), SENTINEL, device="cuda")}
    totals = torch.zeros(5, dtype=torch.float64, device="cuda")
    res = run(enc, pred, W, b, lens, labels, blank, out=out, totals=totals)
    de, dp = res["d_enc"].view(T, 2, J), res["d_pred"].view(Umax + 1, 2, J)
    assert float(res["loss"][1]) == 0.0 and bits(res["loss"])[0] == bits(alone["loss"])[0]
    assert np.array_equal(bits(de[:, 0]), bits(alone["d_enc"])) and np.array_equal(bits(dp[:, 0]), bits(alone["d_pred"]))
    assert np.array_equal(bits(res["W_grad"]), bits(alone["W_grad"]))
    fill = 0.0 if how == "idle" else SENTINEL            # idle: zeros; rejected: untouched
    assert bool((de[:, 1] == fill).all()) and bool((dp[:, 1] == fill).all())
    assert totals.cpu().numpy()[1:].tolist() == ([T, 3, 1, 0] if how == "idle" else [T, 3, 2, 1])


def test_limits_and_argument_errors_leave_the_outputs_alone():
    import kaldi_lstm_amd as k
    lib = k.load_library()
    T, S, Umax, J, V = 4, 1, 2, 16, 5
    x = lambda *shape: torch.full(shape, SENTINEL, device="cuda")
    enc, pred, W, b, de, dp, Wg, bg, loss = x(T, J), x(Umax + 1, J), x(V, J), x(V), x(T, J), x(Umax + 1, J), x(V, J), x(V), x(S)
    lens, (lab, off, _) = torch.tensor([T], dtype=torch.int32, device="cuda"), k.ctc.pack_labels([[1, 2]], "cuda")
    nbytes = k.rnnt_workspace_bytes(T, S, Umax, J, V)
    ws = torch.zeros(nbytes + 256, dtype=torch.uint8, device="cuda")

    def call(**kw):
        a = dict(enc=enc.data_ptr(), es=J, T=T, S=S, Umax=Umax, J=J, V=V, blank=0, ws=ws.data_ptr(), nbytes=nbytes, ds=J)
        a.update(kw)
        return lib.krnnt_eval(a["enc"], a["es"], pred.data_ptr(), J, W.data_ptr(), b.data_ptr(), a["T"], a["S"], a["Umax"], a["J"], a["V"], lens.data_ptr(),
                              lab.data_ptr(), off.data_ptr(), a["blank"], de.data_ptr(), a["ds"], dp.data_ptr(), J, Wg.data_ptr(), bg.data_ptr(),
                              loss.data_ptr(), None, a["ws"], ctypes.c_size_t(a["nbytes"]), None)

    for kw in (dict(S=33), dict(T=0), dict(Umax=1024), dict(T=1 << 20, Umax=1023), dict(J=24), dict(J=1040), dict(V=1), dict(V=4097), dict(blank=V)):
        assert call(**kw) == 2, kw                       # KLSTM_ERR_SHAPE
    for kw in (dict(enc=None), dict(es=J - 1), dict(ds=J - 1), dict(nbytes=nbytes - 1), dict(ws=ws.data_ptr() + 4), dict(enc=enc.data_ptr() + 2)):
        assert call(**kw) == 1, kw                       # KLSTM_ERR_ARG
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in (de, dp, Wg, bg, loss)) and not ws.any()
    assert call() == 0 and np.isfinite(loss.cpu().numpy()).all()


def test_workspace_is_the_documented_formula():
    import kaldi_lstm_amd as k
    up = lambda v: (v + 255) // 256 * 256

    def formula(T, S, Umax, J, V):
        N, tb, splits = S * T * (Umax + 1), (T + 15) // 16, k.rnnt_grad_splits(J, V)
        nodes = up(16 * S) + up(8 * S) + up(16 * S * (T + Umax + 1)) + 7 * up(4 * N)
        partials = up(4 * 4 * S * T * J) + up(4 * tb * S * (Umax + 1) * J) + up(4 * splits * V * J) + up(8 * splits * V)
        return nodes, partials

    for shape in ((500, 8, 50, 512, 64), (33, 3, 16, 48, 130)):
        nodes, partials = formula(*shape)
        assert k.rnnt_workspace_bytes(*shape) == nodes + partials and k.rnnt_workspace_bytes(*shape, want_grads=False) == nodes
        T, S, Umax, J, V = shape
        for bigger in ((T, S, Umax, 2 * J, V), (T, S, Umax, J, 2 * V)):      # V and J reach the partials' term only
            assert k.rnnt_workspace_bytes(*bigger) - formula(*bigger)[1] == nodes
    assert k.rnnt_grad_splits(512, 64) == 256 and k.rnnt_grad_splits(512, 1024) == 32 and k.rnnt_grad_splits(1024, 4096) == 8


@pytest.mark.parametrize("embed", [False, True])
def test_pack_is_the_one_hot_or_the_gather(embed):
    import kaldi_lstm_amd as k
    S, V, bos, D = 3, 7, 6, 5
    labels = [[1, 2, 2, 5], [], [0, 3]]
    rng = np.random.RandomState(1)
    E, eb = rng.randn(D, V).astype(f32), rng.randn(D).astype(f32)
    want = np.zeros((5, S, D if embed else V), f32)
    for s, y in enumerate(labels):
        for u, x in enumerate([bos] + y):
            want[u, s] = E[:, x] + eb if embed else np.eye(V, dtype=f32)[x]
    got = k.rnnt_pack(labels, S, V, bos, embed=torch.from_numpy(E).cuda() if embed else None, bias=torch.from_numpy(eb).cuda() if embed else None)
    assert np.array_equal(bits(got), bits(want.reshape(5 * S, -1)))


EPOCHS = 12


def test_trainer_learns_and_its_first_minibatch_is_the_direct_call():
    """tests/cpp/rnnt_test.cpp train: EPOCHS passes of TrainTransducerWholeUtterances over four utterances, two streams (2 minibatches
    per pass, 24 in all) from a fixed seed.  The first minibatch's losses and joint gradient are krnnt_eval's on the same activations,
    bit for bit; every loss is finite; the last pass's average loss is below the first's."""
    head, losses = cpp_driver.run("rnnt_test", "train", EPOCHS).stdout.split("|")
    avg = [float(v) for v in losses.split()]
    print("average loss per pass:", avg, flush=True)
    assert head.split() == ["OK", "1", "1", str(2 * EPOCHS)]
    assert len(avg) == EPOCHS and all(math.isfinite(v) for v in avg) and avg[-1] < avg[0]


def test_joint_round_trips_through_text_and_binary():
    assert cpp_driver.run("rnnt_test", "io").stdout.split() == ["OK", "1"]
