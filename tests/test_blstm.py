"""The bidirectional layer, host side (no GPU): the numpy twin of klstm_reverse_streams' semantics, the float64 BLSTM truth that
tests/test_blstm_gpu.py measures the engine against (checked here by finite differences), and the host-side checks of
include/klstm_blstm.hpp through tests/cpp/blstm_test."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import kaldi_fmt, ref_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "blstm_test")
SRC = EXE + ".cpp"
HDRS = [os.path.join(ROOT, "include", h) for h in ("klstm.h", "klstm_component.hpp", "klstm_kaldi_io.hpp", "klstm_trainer.hpp",
                                                   "klstm_nnet.hpp", "klstm_blstm.hpp")]

SET, ADD, ZERO_PAD, MASK_COPY = 0, 1, 2, 3


def build_blstm_driver():
    import kaldi_lstm_amd as k
    lib = k.lib_path()
    assert os.path.exists(lib), "libklstm.so missing: run __graft_entry__.build()"
    stale = (not os.path.exists(EXE)) or any(os.path.getmtime(f) > os.path.getmtime(EXE) for f in [SRC] + HDRS)
    if stale:
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), SRC,
                               "-L" + os.path.dirname(lib), "-lklstm", "-Wl,-rpath,$ORIGIN/../../kaldi-lstm_amd", "-o", EXE])
    return EXE


def run(*args, ok=True):
    r = subprocess.run([build_blstm_driver()] + [str(a) for a in args], capture_output=True, text=True, timeout=900)
    if ok:
        assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    return r


# ---------------------------------------------------------------------------------------------------------------------------------
# the numpy twin of klstm_reverse_streams and the float64 truth
# ---------------------------------------------------------------------------------------------------------------------------------
def reverse_np(x, lens, T, out, mode):
    """out [T*S, cols] (modified in place and returned) from x [T*S, cols]; row t*S + s; lens clamped to [0, T] as the kernel does."""
    S = len(lens)
    for s in range(S):
        n = min(max(int(lens[s]), 0), T)
        for t in range(T):
            row = t * S + s
            if t >= n:
                if mode != ADD:
                    out[row] = 0
            elif mode == SET:
                out[row] = x[(n - 1 - t) * S + s]
            elif mode == ADD:
                out[row] = out[row] + x[(n - 1 - t) * S + s]
            elif mode == MASK_COPY:
                out[row] = x[row]
    return out


def pad_mask(lens, T):
    """[T*S] bool: True on the valid rows"""
    S = len(lens)
    return np.array([(r // S) < lens[r % S] for r in range(T * S)])


def blstm_truth(pf, pb, x, od, lens, I, C, R):
    """float64 BLSTM on whole utterances, per stream and direction on the valid prefix with S = 1 (tests/ref_torch.py).  Returns
    out [T*S, 2R], in_diff [T*S, I], grad_f, grad_b (summed over streams; padding rows of out / in_diff zero)."""
    S = len(lens)
    T = x.shape[0] // S
    out = np.zeros((T * S, 2 * R))
    ind = np.zeros((T * S, I))
    gf, gb = np.zeros(pf.size), np.zeros(pb.size)
    z = (np.zeros((1, C)), np.zeros((1, R)))
    for s in range(S):
        n = int(lens[s])
        if n == 0:
            continue
        xs = np.asarray(x[s::S][:n], np.float64)
        ods = np.asarray(od[s::S][:n], np.float64)
        of, g, dx, _, _ = ref_torch.grads(pf.astype(np.float64), xs, ods[:, :R], *z, I, C, R, 1)
        ob, g2, dx2, _, _ = ref_torch.grads(pb.astype(np.float64), xs[::-1].copy(), ods[::-1, R:].copy(), *z, I, C, R, 1)
        rows = np.arange(n) * S + s
        out[rows, :R], out[rows, R:] = of, ob[::-1]
        ind[rows] = dx + dx2[::-1]
        gf += g
        gb += g2
    return out, ind, gf, gb


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the twin's semantics
# ---------------------------------------------------------------------------------------------------------------------------------
def test_reverse_twin_semantics():
    T, S, cols = 5, 3, 2
    lens = [5, 2, 0]
    x = np.arange(T * S * cols, dtype=np.float64).reshape(T * S, cols)
    out = reverse_np(x, lens, T, np.full_like(x, -1.0), SET)
    for t in range(T):
        np.testing.assert_array_equal(out[t * S + 0], x[(4 - t) * S + 0])
    np.testing.assert_array_equal(out[0 * S + 1], x[1 * S + 1])
    np.testing.assert_array_equal(out[1 * S + 1], x[0 * S + 1])
    assert (out[2 * S + 1::S] == 0).all() and (out[2::S] == 0).all()
    # an involution on the valid rows; ADD leaves padding alone; ZERO_PAD touches only padding; MASK_COPY is the masked identity
    twice = reverse_np(out, lens, T, np.zeros_like(x), SET)
    m = pad_mask(lens, T)
    np.testing.assert_array_equal(twice[m], x[m])
    added = reverse_np(x, lens, T, np.full_like(x, 7.0), ADD)
    np.testing.assert_array_equal(added[~m], 7.0)
    np.testing.assert_array_equal(added[m], out[m] + 7.0)
    z = reverse_np(None, lens, T, x.copy(), ZERO_PAD)
    np.testing.assert_array_equal(z[m], x[m])
    assert (z[~m] == 0).all()
    mc = reverse_np(x, lens, T, np.full_like(x, -1.0), MASK_COPY)
    np.testing.assert_array_equal(mc[m], x[m])
    assert (mc[~m] == 0).all()
    # lengths outside [0, T] are clamped
    np.testing.assert_array_equal(reverse_np(x, [9, -3, 0], T, np.zeros_like(x), SET), reverse_np(x, [5, 0, 0], T, np.zeros_like(x), SET))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the float64 truth against finite differences, and its padding rules
# ---------------------------------------------------------------------------------------------------------------------------------
def _small():
    I, C, R, S, T = 3, 4, 2, 3, 6
    rng = np.random.RandomState(5)
    n = 4 * C * I + 4 * C * R + 4 * C + 3 * C + R * C
    pf, pb = rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n)
    x = rng.randn(T * S, I)
    od = rng.randn(T * S, 2 * R)
    return I, C, R, S, T, pf, pb, x, od, [6, 3, 0]


def _objective(pf, pb, x, od, lens, I, C, R):
    out = blstm_truth(pf, pb, x, od, lens, I, C, R)[0]
    return float((out * od * pad_mask(lens, x.shape[0] // len(lens))[:, None]).sum())


def test_blstm_truth_finite_differences():
    I, C, R, S, T, pf, pb, x, od, lens = _small()
    out, ind, gf, gb = blstm_truth(pf, pb, x, od, lens, I, C, R)
    m = pad_mask(lens, T)
    assert (out[~m] == 0).all() and (ind[~m] == 0).all()
    rng = np.random.RandomState(0)
    eps = 1e-6

    def fd(fn, v, idx):
        a, b = v.copy(), v.copy()
        a.flat[idx] += eps
        b.flat[idx] -= eps
        return (fn(a) - fn(b)) / (2 * eps)

    for idx in rng.choice(pf.size, 12, replace=False):
        assert abs(fd(lambda p: _objective(p, pb, x, od, lens, I, C, R), pf, idx) - gf[idx]) <= 1e-6 * max(1.0, abs(gf[idx]))
        assert abs(fd(lambda p: _objective(pf, p, x, od, lens, I, C, R), pb, idx) - gb[idx]) <= 1e-6 * max(1.0, abs(gb[idx]))
    for idx in rng.choice(np.flatnonzero(np.repeat(m, I)), 12, replace=False):
        assert abs(fd(lambda v: _objective(pf, pb, v, od, lens, I, C, R), x, idx) - ind.flat[idx]) <= 1e-6 * max(1.0, abs(ind.flat[idx]))


def test_blstm_truth_padding_is_inert():
    """Garbage in the padding rows of x and out_diff changes nothing; the backward half of a full-length stream is the forward
    recurrence on the reversed utterance."""
    I, C, R, S, T, pf, pb, x, od, lens = _small()
    m = pad_mask(lens, T)
    ref = blstm_truth(pf, pb, x, od, lens, I, C, R)
    x2, od2 = x.copy(), od.copy()
    x2[~m], od2[~m] = 1e3, -1e3
    for a, b in zip(ref, blstm_truth(pf, pb, x2, od2, lens, I, C, R)):
        np.testing.assert_array_equal(a, b)
    xs = torch.tensor(x[0::S][::-1].copy())
    ob = ref_torch.forward(torch.tensor(pb), xs, torch.zeros(1, C, dtype=torch.float64), torch.zeros(1, R, dtype=torch.float64),
                           I, C, R, 1)[0].numpy()
    np.testing.assert_allclose(ref[0][0::S, R:], ob[::-1], rtol=0, atol=1e-14)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the C++ layer's host-side checks (tests/cpp/blstm_test; no device memory is touched)
# ---------------------------------------------------------------------------------------------------------------------------------
def _models(tmp_path, I=8, C=16, R=8, S=4, I2=None, C2=None, S2=None, marker2="<LstmProjectedStreams>"):
    from oracle.oracle import make_params
    pf = make_params(I, C, R, scale=0.1, seed=1)
    I2, C2, S2 = I2 or I, C2 or C, S2 or S
    pb = make_params(I2, C2, R, scale=0.1, seed=2)
    (tmp_path / "f.bin").write_bytes(kaldi_fmt.binary_model(pf, I, C, R, S))
    (tmp_path / "b.bin").write_bytes(kaldi_fmt.binary_model(pb, I2, C2, R, S2, marker=marker2))
    return tmp_path / "f.bin", tmp_path / "b.bin", pf, pb


def test_layer_shape(tmp_path):
    f, b, pf, pb = _models(tmp_path)
    assert run("shape", f, b).stdout.split() == ["OK", "8", "16", str(pf.size + pb.size)]


@pytest.mark.parametrize("what", ["input", "cell", "streams", "standard"])
def test_layer_refuses_mismatched_directions(tmp_path, what):
    kw = {"input": dict(I2=12), "cell": dict(C2=24), "streams": dict(S2=2), "standard": dict(marker2="<LstmProjected>")}[what]
    f, b, _, _ = _models(tmp_path, **kw)
    r = run("shape", f, b, ok=False)
    assert r.returncode == 1 and r.stdout.startswith("ERROR") and "BLstmProjectedStreams" in r.stdout, r.stdout


def test_layer_has_no_model_file_form(tmp_path):
    f, b, _, _ = _models(tmp_path)
    r = run("write", f, b, ok=False)
    assert r.returncode == 1 and "no model-file form" in r.stdout, r.stdout


@pytest.mark.parametrize("lens", ["4,4,4", "4,4,-1,4"])
def test_seq_lengths_checked(tmp_path, lens):
    f, b, _, _ = _models(tmp_path)
    r = run("seqlens", f, b, lens, ok=False)
    assert r.returncode == 1 and "SetSeqLengths" in r.stdout, r.stdout
