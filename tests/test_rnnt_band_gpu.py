"""Band-pruned transducer training on the GPU (krnnt_band_eval, krnnt_band_from_frames of include/klstm_rnnt.h) against
tests/rnnt_band_ref.py, and the C++ layer over them (Transducer::EvalBanded / BandFromFrames, the band option of
TrainTransducerWholeUtterances) through tests/cpp/rnnt_band_test.cpp.

Parity: the measure and the bar of tests/test_rnnt_gpu.py, imported from there unchanged: max|gpu - truth64| / max|truth64| per tensor
through margins.bound(), bar = max(4 x the error of the float32 twin on the same inputs, 2^-22).  The measured figures are in
profiles/rnnt_band_margins.json and DESIGN.md 4za.  The shapes sit at the edges of the banded tiles (klstm_rnnt_band.hip: 16 frames x 8
band offsets per forward tile, 4 offsets per backward step, 128 classes per pass, 128 columns per owner round of the backward epilogue,
one wave of 64 lanes per lattice direction, three instances of the backward kernel by J); the table of the issue needed no change."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import cpp_driver, rnnt_band_ref, rnnt_ref
from tests.test_rnnt_gpu import SENTINEL, TENSORS, bits, check, padding_intact, placed

pytestmark = pytest.mark.gpu
f32 = np.float32


def band_rule(Ts, U, R, left, frames=None):
    """the rule of krnnt_band_from_frames for one stream, transcribed"""
    hi = max(0, U + 1 - R)
    c = [t * U // Ts if frames is None else sum(f < t for f in frames) for t in range(Ts)]
    u0 = [min(max(ci - left, 0), hi) for ci in c]
    u0[-1] = hi
    for t in range(Ts - 2, -1, -1):
        u0[t] = max(u0[t], u0[t + 1] - (R - 1))
    ok = u0[0] == 0 and (frames is None or (all(0 <= f < Ts for f in frames) and list(frames) == sorted(frames)))
    return u0 if ok else [-1] * Ts


def valid(u0, U, R):
    return u0[0] == 0 and all(0 <= b - a <= R - 1 for a, b in zip(u0, u0[1:])) and u0[-1] <= U <= u0[-1] + R - 1


# (T, Umax, V, J, S, R, band, left (None: (R-1)//2), blank is V - 1)
CASES = [(1, 0, 2, 16, 1, 1, "zero", None, 0), (5, 3, 17, 16, 1, 2, "linear", 0, 1), (17, 5, 17, 48, 1, 8, "zero", None, 0),
         (16, 20, 129, 48, 1, 8, "slope", None, 1), (17, 8, 17, 48, 3, 4, "frames", None, 0), (33, 16, 130, 16, 3, 9, "frames", 0, 1),
         (33, 16, 130, 16, 3, 9, "frames", 8, 0), (40, 70, 5, 16, 1, 33, "linear", None, 1), (5, 4, 5, 144, 1, 3, "linear", 0, 0),
         (3, 2, 5, 528, 1, 2, "linear", 0, 1)]


@functools.lru_cache(maxsize=None)
def problem(T, Umax, V, J, S, R, kind, left, blank_last, seed=0):
    """inputs (ragged at S = 3: a repeated label at full length, U = 0, T_s < T), a valid band of the kind, and both references"""
    rng = np.random.RandomState(seed + 7 * T + Umax)
    blank = V - 1 if blank_last else 0
    enc, pred = rng.randn(T * S, J).astype(f32), rng.randn((Umax + 1) * S, J).astype(f32)
    W, b = rng.uniform(-0.3, 0.3, (V, J)).astype(f32), rng.uniform(-0.3, 0.3, V).astype(f32)
    lens, ulen = [T] * S, [Umax] * S
    if S == 3:
        lens, ulen = [T, T, max(T - 1, 1)], [Umax, 0, max(Umax - 1, 0)]
    labels = [[int(v) for v in (rng.randint(0, V - 1, n) + (blank == 0))] for n in ulen]
    if Umax >= 2:
        labels[0][1] = labels[0][0]
    left = (R - 1) // 2 if left is None else left
    band = np.zeros((S, T), np.int32)
    for s in range(S):
        Ts, U = lens[s], ulen[s]
        frames = sorted(int(f) for f in rng.randint(0, Ts, U)) if kind == "frames" else None
        row = {"zero": [0] * Ts, "slope": [min((R - 1) * t, max(0, U + 1 - R)) for t in range(Ts)]}.get(kind) or band_rule(Ts, U, R, left, frames)
        assert valid(row, U, R), (kind, row)
        band[s, :Ts], band[s, Ts:] = row, row[-1]
    refs = [rnnt_band_ref.transducer(enc, pred, W, b, lens, labels, blank, band, R, dt) for dt in (torch.float64, torch.float32)]
    return enc, pred, W, b, lens, labels, blank, band, refs[0], refs[1]


def run(enc, pred, W, b, lens, labels, blank, band, R, **kw):
    import kaldi_lstm_amd as k
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=f32)).cuda()
    return k.rnnt_band_eval(d(enc) if isinstance(enc, np.ndarray) else enc, d(pred) if isinstance(pred, np.ndarray) else pred, d(W), d(b), lens,
                            labels, torch.from_numpy(np.ascontiguousarray(band, dtype=np.int32)).cuda(), R, blank=blank, **kw)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "T%d-U%d-V%d-J%d-S%d-R%d-%s-l%s-b%d" % c)
def test_band_eval_against_float64(case):
    T, Umax, V, J, S, R = case[:6]
    enc, pred, W, b, lens, labels, blank, band, truth, twin = problem(*case)
    (ev, eb), (pv, pb) = placed(enc, 0), placed(pred, 1)
    out = {"d_enc": placed(np.full_like(enc, SENTINEL), 1), "d_pred": placed(np.full_like(pred, SENTINEL), 0)}
    totals = torch.zeros(5, dtype=torch.float64, device="cuda")
    res = run(ev, pv, W, b, lens, labels, blank, band, R, totals=totals, out={k: v[0] for k, v in out.items()})
    torch.cuda.synchronize()
    assert padding_intact(*out["d_enc"], 1) and padding_intact(*out["d_pred"], 0), "columns outside the rows were written"
    check("%s" % (case,), res, truth, twin)
    assert np.allclose(totals.cpu().numpy(), [truth["loss"].sum(), sum(lens), sum(len(y) for y in labels), S, 0], rtol=1e-5)
    if S == 3:                                           # rows t >= T_s of d_enc and u > U_s of d_pred are written as zero
        assert not res["d_pred"].reshape(Umax + 1, S, J)[1:, 1].any() and not res["d_enc"].reshape(T, S, J)[T - 1, 2].any()
    if R >= Umax + 1 and not band.any():                 # the whole lattice is in band: the full definition's references hold as well
        check("%s full" % (case,), res, *[rnnt_ref.transducer(enc, pred, W, b, lens, labels, blank, dt) for dt in (torch.float64, torch.float32)])


def test_long_banded_lattice_keeps_its_digits():
    """T = 400, U = 60, R = 8 around the straight line: log alpha reaches -400; the same bar holds because the recursion runs in double
    and the planes are stored relative to offsets summed in double"""
    rng = np.random.RandomState(5)
    T, U, J, V, R = 400, 60, 16, 4, 8
    enc, pred = rng.randn(T, J).astype(f32), rng.randn(U + 1, J).astype(f32)
    W, b = rng.uniform(-0.3, 0.3, (V, J)).astype(f32), rng.uniform(-0.3, 0.3, V).astype(f32)
    y, band = [[int(v) for v in rng.randint(1, V, U)]], np.array([band_rule(T, U, R, 3)], np.int32)
    truth, twin = [rnnt_band_ref.transducer(enc, pred, W, b, [T], y, 0, band, R, dt) for dt in (torch.float64, torch.float32)]
    check("long", run(enc, pred, W, b, [T], y, 0, band, R), truth, twin)


def test_runs_and_stream_company_leave_the_bits_alone():
    case = (17, 8, 17, 48, 3, 4, "frames", None, 0)
    T, Umax, V, J, S, R = case[:6]
    enc, pred, W, b, lens, labels, blank, band = problem(*case)[:8]
    one, two, fwd = [run(enc, pred, W, b, lens, labels, blank, band, R, want_grads=g) for g in (True, True, False)]
    for name in TENSORS:
        assert np.array_equal(bits(one[name]), bits(two[name])), f"{name}: two runs differ"
    assert np.array_equal(bits(one["loss"]), bits(fwd["loss"])) and set(fwd) == {"loss"}
    e3, p3 = enc.reshape(T, S, J), pred.reshape(Umax + 1, S, J)
    for order in ([0], [1], [2], [2, 0, 1]):
        sub = run(e3[:, order].reshape(-1, J), p3[:, order].reshape(-1, J), W, b, [lens[s] for s in order], [labels[s] for s in order], blank,
                  band[order], R)
        n = len(order)
        for i, s in enumerate(order):
            assert bits(sub["loss"])[i] == bits(one["loss"])[s]
            assert np.array_equal(bits(sub["d_enc"].view(T, n, J)[:, i]), bits(one["d_enc"].view(T, S, J)[:, s])), (order, s)
            assert np.array_equal(bits(sub["d_pred"].view(Umax + 1, n, J)[:, i]), bits(one["d_pred"].view(Umax + 1, S, J)[:, s])), (order, s)


@pytest.mark.parametrize("how", ["u0(0) = 1", "a jump of R", "the end misses U"])
def test_a_stream_with_an_invalid_band_is_rejected(how):
    T, Umax, V, J, R = 9, 3, 5, 16, 2
    rng = np.random.RandomState(3)
    enc, pred = rng.randn(T * 2, J).astype(f32), rng.randn((Umax + 1) * 2, J).astype(f32)
    W, b = rng.uniform(-0.3, 0.3, (V, J)).astype(f32), rng.uniform(-0.3, 0.3, V).astype(f32)
    lens, labels, good = [T, T], [[1, 2, 3], [2, 1, 4]], band_rule(T, 3, R, 0)
    bad = {"u0(0) = 1": [1] + good[1:], "a jump of R": [0] * 4 + [2] * 5, "the end misses U": [0] * 8 + [1]}[how]
    assert valid(good, 3, R) and not valid(bad, 3, R)
    alone = run(enc.reshape(T, 2, J)[:, 0], pred.reshape(Umax + 1, 2, J)[:, 0], W, b, [T], [labels[0]], 0, np.array([good]), R)
    out = {"d_enc": torch.full((T * 2, J), SENTINEL, device="cuda"), "d_pred": torch.full(((Umax + 1) * 2, J), SENTINEL, device="cuda")}
    totals = torch.zeros(5, dtype=torch.float64, device="cuda")
    res = run(enc, pred, W, b, lens, labels, 0, np.array([good, bad]), R, out=out, totals=totals)
    de, dp = res["d_enc"].view(T, 2, J), res["d_pred"].view(Umax + 1, 2, J)
    assert float(res["loss"][1]) == 0.0 and bits(res["loss"])[0] == bits(alone["loss"])[0]
    assert np.array_equal(bits(de[:, 0]), bits(alone["d_enc"])) and np.array_equal(bits(dp[:, 0]), bits(alone["d_pred"]))
    assert np.array_equal(bits(res["W_grad"]), bits(alone["W_grad"]))
    assert bool((de[:, 1] == SENTINEL).all()) and bool((dp[:, 1] == SENTINEL).all())
    assert totals.cpu().numpy()[1:].tolist() == [T, 3, 2, 1]


@pytest.mark.parametrize("R,left,with_frames", [(4, None, True), (9, 0, True), (9, 8, True), (1, None, False), (6, 2, False), (64, None, True)])
def test_band_from_frames_is_the_rule(R, left, with_frames):
    """against band_rule(): streams across the chunk of 256 frames of the kernel's scan, U = 0, an idle stream, a stream no band of width R
    can serve (a row of -1), one with frames out of order (-1 as well); every band produced is valid"""
    import kaldi_lstm_amd as k
    rng = np.random.RandomState(R)
    lens, ulen = [600, 257, 40, 0, 9, 30], [70, 300, 0, 0, 9 * R, 12]
    labels = [[1] * n for n in ulen]
    frames = [sorted(int(f) for f in rng.randint(0, max(Ts, 1), n)) for Ts, n in zip(lens, ulen)] if with_frames else None
    if with_frames:
        frames[5][3], frames[5][4] = 20, 19
    got = k.rnnt_band_from_frames(lens, labels, R, frames=frames, left=left).cpu().numpy()
    assert got.shape == (6, 600)
    for s, (Ts, U) in enumerate(zip(lens, ulen)):
        want = band_rule(Ts, U, R, (R - 1) // 2 if left is None else left, frames[s] if with_frames else None) if Ts else []
        assert got[s, :Ts].tolist() == want, s
        assert (got[s, Ts:] == (want[-1] if Ts else 0)).all() and (want[:1] in ([], [-1]) or valid(want, U, R)), s
    assert got[4, 0] == -1 and (not with_frames or got[5, 0] == -1)


def test_the_cpp_holder_is_the_python_path_and_the_banded_trainer_learns():
    """tests/cpp/rnnt_band_test.cpp.  eval: Transducer::BandFromFrames + EvalBanded on inputs from a 32-bit generator that is repeated
    here; the losses and the sums of the gradients' bits are those of rnnt_band_from_frames + rnnt_band_eval.  train: two passes of
    TrainTransducerWholeUtterances with band = 4 lower the loss; with band = 0 every minibatch is krnnt_eval's, bit for bit."""
    import kaldi_lstm_amd as k
    T, Umax, V, J, S, R = 21, 6, 7, 32, 2, 4
    state = [12345]

    def gen(n):
        out = np.empty(n, f32)
        for i in range(n):
            state[0] = (state[0] * 1664525 + 1013904223) & 0xFFFFFFFF
            out[i] = ((state[0] >> 8) & 0xFFFF) / 65536.0 - 0.5
        return torch.from_numpy(out).cuda()

    enc, pred, W, b = gen(T * S * J).view(T * S, J), gen((Umax + 1) * S * J).view(-1, J), gen(V * J).view(V, J), gen(V)
    lens, labels, frames = [T, T - 4], [[1, 2, 2, 3, 4, 6], [5, 1, 3]], [[1, 4, 5, 9, 14, 18], [0, 7, 11]]
    band = k.rnnt_band_from_frames(lens, labels, R, frames=frames, T=T)
    res = k.rnnt_band_eval(enc, pred, W, b, lens, labels, band, R)
    want = [int(v) for v in bits(res["loss"])] + [int(bits(res[n]).astype(np.uint64).sum()) for n in ("d_enc", "d_pred", "W_grad", "b_grad")]
    got = cpp_driver.run("rnnt_band_test", "eval").stdout.split()
    assert got[0] == "OK" and [int(v) for v in got[1:]] == want
    head, losses = cpp_driver.run("rnnt_band_test", "train").stdout.split("|")
    avg = [float(v) for v in losses.split()]
    print("banded trainer, average loss per pass:", avg, flush=True)
    assert head.split() == ["OK", "1"] and len(avg) == 2 and np.isfinite(avg).all() and avg[1] < avg[0]
