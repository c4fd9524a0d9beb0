"""The bidirectional layer on the device: klstm_reverse_streams against its numpy twin bit for bit, kaldi_lstm_amd.BidirectionalLstm
against the float64 truth of tests/test_blstm.py (per stream and direction on the valid prefix, S = 1) at trained-size weights, padding
that changes nothing, the wrapper against a plain Engine fed the host-built reversal, and the C++ layer (include/klstm_blstm.hpp through
tests/cpp/blstm_test) against the Python path bit for bit.

Bar, per tensor: relerr(engine, fp64) <= max(4 relerr(fp32 oracle, fp64), floor), relerr = max |a - b| / max |b| over the valid rows --
the ratio of tests/test_trained_regime_gpu.py.  (A ratio of 3 does not hold for the engines themselves: over these 100-frame
utterances two gradient tensors measured 3.6x and 3.8x the fp32 oracle's error, and the wrapper is bit-identical to two plain engines,
test_wrapper_equals_plain_engines.)  Floors: 1e-5 for out; 4e-5 for in_diff, the momentum buffers and the parameter changes
theta_k - theta_0 (lr times sums of those buffers): twice the 2e-5 of the 20-frame minibatches there, for sums over up to 100
frames per stream.  The fp32 oracle (oracle.Oracle) runs the same minibatches on the
host-built padded and reversed inputs.  Margins go to parity_margins.json through tests.margins.bound."""
import numpy as np
import pytest
import torch

import kaldi_lstm_amd as k
from oracle.oracle import Oracle, split_blob
from tests import kaldi_fmt
from tests import regimes as rg
from tests.margins import bound
from tests.test_blstm import ADD, MASK_COPY, SET, ZERO_PAD, blstm_truth, pad_mask, reverse_np, run

pytestmark = pytest.mark.gpu

K = 4.0
FLOOR_FWD, FLOOR_BWD = 1e-5, 4e-5
LR, MOM = rg.LR, rg.MOMENTUM


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def relerr(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / (np.abs(b).max() + 1e-30))


def check(name, eng, f32, f64, floor):
    e32, een = relerr(f32, f64), relerr(eng, f64)
    bound(een, max(K * e32, floor), name)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the reversal kernel against numpy, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [37, 40, 512])
@pytest.mark.parametrize("T", [1, 7, 50])
@pytest.mark.parametrize("S", [1, 3, 4, 16])
def test_reverse_streams_kernel(S, T, cols):
    rng = np.random.RandomState(S * 1000 + T * 10 + cols)
    pool = [0, 1, T] + list(rng.randint(0, T + 1, 16))
    lens = np.array([pool[(s + T) % len(pool)] for s in range(S)], np.int32)
    ld = torch.from_numpy(lens).cuda()
    rows = T * S
    src = rng.randn(rows, 2 * cols).astype(np.float32)           # column windows: offset cols, stride 2 cols
    x = cuda(src)
    for mode in (SET, ADD, ZERO_PAD, MASK_COPY):
        dst0 = rng.randn(rows, 2 * cols).astype(np.float32)
        out = cuda(dst0)
        k.reverse_streams(None if mode == ZERO_PAD else x[:, cols:], ld, T, out[:, cols:], mode)
        want = dst0.copy()
        reverse_np(src[:, cols:], lens, T, want[:, cols:], mode)
        got = out.cpu().numpy()
        assert np.array_equal(got, want), (mode, np.argwhere(got != want)[:4].tolist())
        # a contiguous block too (the float4 path where cols allows it)
        out2 = cuda(dst0[:, :cols])
        k.reverse_streams(None if mode == ZERO_PAD else cuda(src[:, :cols]), ld, T, out2, mode)
        assert np.array_equal(out2.cpu().numpy(), reverse_np(src[:, :cols], lens, T, dst0[:, :cols].copy(), mode)), mode


def test_reverse_streams_arguments():
    ld = torch.tensor([2, 1], dtype=torch.int32, device="cuda")
    x = torch.zeros(6, 5, device="cuda")
    lib = k.load_library()
    assert lib.klstm_reverse_streams(x.data_ptr(), 5, 2, 3, 5, ld.data_ptr(), x.data_ptr(), 5, SET, None) == 1    # in == out
    assert lib.klstm_reverse_streams(x.data_ptr(), 5, 2, 3, 5, ld.data_ptr(), None, 5, SET, None) == 1
    assert lib.klstm_reverse_streams(x.data_ptr(), 4, 2, 3, 5, ld.data_ptr(), x.data_ptr(), 5, MASK_COPY, None) == 1   # stride < cols
    assert lib.klstm_reverse_streams(x.data_ptr(), 5, 2, 3, 5, ld.data_ptr(), x.data_ptr(), 5, 4, None) == 1     # mode
    assert lib.klstm_reverse_streams(x.data_ptr(), 5, 0, 3, 5, ld.data_ptr(), x.data_ptr(), 5, SET, None) == 1     # S
    assert lib.klstm_reverse_streams(None, 0, 2, 0, 5, None, None, 5, SET, None) == 0                              # rows == 0
    assert lib.klstm_reverse_streams(x.data_ptr(), 5, 1 << 16, 1 << 16, 5, ld.data_ptr(), x.data_ptr(), 5, MASK_COPY, None) == 2


# ---------------------------------------------------------------------------------------------------------------------------------
# the runs
# ---------------------------------------------------------------------------------------------------------------------------------
def lens_for(S, T):
    base = [T, T - 13, 57, 1, T - 1, 0, 71, T - 30]
    return base[:S]


def inputs(I, R, T, S, lens, rng):
    x, od = rg.trained_inputs(I, 2 * R, T, S, rng)
    od[~pad_mask(lens, T)] = 0
    return x, od


def blstm_minibatch(bl, x, od, lens, flags=0, want_in_diff=True, lr=LR):
    S, R, I = bl.S, bl.R, bl.I
    rows = x.shape[0]
    xd, odd = cuda(x), cuda(od)
    out = torch.full((rows, 2 * R), float("nan"), device="cuda")
    ind = torch.full((rows, I), float("nan"), device="cuda") if want_in_diff else None
    torch.cuda.synchronize()
    bl.propagate(xd, lens, out)
    bl.backpropagate(xd, odd, in_diff=ind, momentum=MOM, flags=flags)
    bl.update(lr)
    bl.synchronize()
    torch.cuda.synchronize()
    return out.cpu().numpy(), ind.cpu().numpy() if want_in_diff else None


def oracle_minibatch(of, ob, x, od, lens, R, lr=LR):
    """the fp32 oracle on the host-built inputs: padding rows of x zero for both directions, out_diff masked"""
    T = x.shape[0] // len(lens)
    m = pad_mask(lens, T)
    xz = np.where(m[:, None], x, 0).astype(of.dtype)
    xr = reverse_np(x, lens, T, np.zeros_like(xz), SET)
    odf = np.where(m[:, None], od[:, :R], 0).astype(of.dtype)
    odb = reverse_np(od[:, R:], lens, T, np.zeros_like(odf), SET)
    S = len(lens)
    for o in (of, ob):
        o.reset(np.ones(S, np.int32))
    outf = of.propagate(xz)
    outb = ob.propagate(xr)
    indf = of.backpropagate(xz, odf, momentum=MOM)
    indb = ob.backpropagate(xr, odb, momentum=MOM)
    of.update(lr)
    ob.update(lr)
    out = np.concatenate([outf, reverse_np(outb, lens, T, np.zeros_like(outb), SET)], 1)
    ind = reverse_np(indb, lens, T, indf.copy(), ADD)
    out[~m] = 0
    ind[~m] = 0
    return out, ind


def fp64_minibatch(st, x, od, lens, I, C, R, lr=LR):
    out, ind, gf, gb = blstm_truth(st["pf"], st["pb"], x, od, lens, I, C, R)
    for d, g in (("f", gf), ("b", gb)):
        st["c" + d] = MOM * st["c" + d] + g
        st["p" + d] = st["p" + d] - lr * st["c" + d]
    return out, ind


SHAPES = [(40, 800, 512, 4), (40, 800, 512, 8), (512, 800, 512, 4)]
IDS = ["40-800-512-s4", "40-800-512-s8", "512-800-512-s4"]


def _parity(I, C, R, S, T, nmb, flags=0, want_in_diff=True, seed=11, persistent=True):
    lens = lens_for(S, T)
    pf, pb = rg.trained_params(I, C, R, seed), rg.trained_params(I, C, R, seed + 100)
    bl = k.BidirectionalLstm(I, C, R, S)
    bl.set_params(pf, pb)
    o32 = [Oracle(I, C, R, S, np.float32, threads=8) for _ in range(2)]
    o32[0].set_params(pf)
    o32[1].set_params(pb)
    st = dict(pf=pf.astype(np.float64), pb=pb.astype(np.float64), cf=np.zeros(pf.size), cb=np.zeros(pb.size))
    rng = np.random.RandomState(seed)
    m = None
    try:
        for mb in range(nmb):
            x, od = inputs(I, R, T, S, lens, rng)
            m = pad_mask(lens, T)
            before = [e.profile_query("persist_launches")[1] for e in (bl.fwd, bl.bwd)]
            out_e, ind_e = blstm_minibatch(bl, x, od, lens, flags, want_in_diff)
            out_3, ind_3 = oracle_minibatch(o32[0], o32[1], x, od, lens, R)
            out_6, ind_6 = fp64_minibatch(st, x, od, lens, I, C, R)
            for n, e in enumerate((bl.fwd, bl.bwd)):
                if persistent:
                    assert e.profile_query("persist_launches")[1] > before[n], f"minibatch {mb}: no persistent launch in direction {n}"
                assert e.profile_query("persist_giveups")[1] == 0
            assert (out_e[~m] == 0).all(), "padding rows of out"
            check("out", out_e[m], out_3[m], out_6[m], FLOOR_FWD)
            if want_in_diff:
                assert (ind_e[~m] == 0).all(), "padding rows of in_diff"
                check("in_diff", ind_e[m], ind_3[m], ind_6[m], FLOOR_BWD)
            corr_e, par_e = bl.get_corr(), bl.get_params()
            for d, (eng, o) in enumerate(zip((bl.fwd, bl.bwd), o32)):
                sl = slice(0, pf.size) if d == 0 else slice(pf.size, 2 * pf.size)
                dn = "fb"[d]
                p0 = (pf, pb)[d].astype(np.float64)
                for name, v in split_blob(corr_e[sl], I, C, R).items():
                    check(f"corr{dn}.{name}", v, split_blob(o.get_corr(), I, C, R)[name], split_blob(st["c" + dn], I, C, R)[name], FLOOR_BWD)
                dpe = split_blob(par_e[sl].astype(np.float64) - p0, I, C, R)
                dp3 = split_blob(o.get_params().astype(np.float64) - p0, I, C, R)
                dp6 = split_blob(st["p" + dn] - p0, I, C, R)
                for name in dpe:
                    check(f"dparams{dn}.{name}", dpe[name], dp3[name], dp6[name], FLOOR_BWD)
    finally:
        bl.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. + 3. forward, backward and three Updates against fp64 at trained-size weights
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_blstm_vs_fp64(shape):
    I, C, R, S = shape
    _parity(I, C, R, S, T=100, nmb=3)


def test_blstm_vs_fp64_fused_update():
    _parity(40, 800, 512, 4, T=100, nmb=2, flags=k.binding.BPTT_FUSE_UPDATE)


def test_blstm_vs_fp64_no_in_diff():
    _parity(512, 800, 512, 4, T=100, nmb=2, want_in_diff=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. long whole utterances at a small shape
# ---------------------------------------------------------------------------------------------------------------------------------
def test_blstm_long_utterances():
    _parity(40, 64, 32, 4, T=1000, nmb=1, persistent=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. padding is inert
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 2], ids=["plain", "fused"])
def test_padding_is_inert(flags):
    I, C, R, S, T = 40, 800, 512, 4, 60
    lens = [T, 41, 0, 17]
    m = pad_mask(lens, T)
    pf, pb = rg.trained_params(I, C, R, 1), rg.trained_params(I, C, R, 2)
    rng = np.random.RandomState(3)
    data = [inputs(I, R, T, S, lens, rng) for _ in range(2)]
    res = []
    for garbage in (False, True):
        bl = k.BidirectionalLstm(I, C, R, S)
        bl.set_params(pf, pb)
        g = np.random.RandomState(9)
        outs = []
        for x, od in data:
            x, od = x.copy(), od.copy()
            x[~m] = g.uniform(-1e3, 1e3, x[~m].shape) if garbage else 0
            od[~m] = g.uniform(-1e3, 1e3, od[~m].shape) if garbage else 0
            outs += list(blstm_minibatch(bl, x, od, lens, flags))
        outs += [bl.get_params(), bl.get_corr()]
        res.append(outs)
        bl.close()
    for n, (a, b) in enumerate(zip(*res)):
        assert np.array_equal(a, b), f"tensor {n} differs: {np.abs(a - b).max()}"


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the wrapper adds nothing numerically
# ---------------------------------------------------------------------------------------------------------------------------------
def test_wrapper_equals_plain_engines():
    I, C, R, S, T = 40, 800, 512, 8, 80
    lens = lens_for(S, T)
    m = pad_mask(lens, T)
    pf, pb = rg.trained_params(I, C, R, 4), rg.trained_params(I, C, R, 5)
    x, od = inputs(I, R, T, S, lens, np.random.RandomState(6))
    bl = k.BidirectionalLstm(I, C, R, S)
    bl.set_params(pf, pb)
    out, ind = blstm_minibatch(bl, x, od, lens)
    ef, eb = k.Engine(I, C, R, S), k.Engine(I, C, R, S)
    ef.set_params(pf)
    eb.set_params(pb)
    xr = reverse_np(x, lens, T, np.zeros_like(x), SET)
    odf = np.where(m[:, None], od[:, :R], 0)
    odb = reverse_np(od[:, R:], lens, T, np.zeros_like(odf), SET)
    res = []
    for e, xx, oo in ((ef, x, odf), (eb, xr, odb)):
        xd, odd = cuda(xx), cuda(oo)
        o, i = torch.empty(T * S, R, device="cuda"), torch.empty(T * S, I, device="cuda")
        e.propagate(xd, o)
        e.backpropagate(xd, odd, i, momentum=MOM)
        e.update(LR)
        e.synchronize()
        res.append((o.cpu().numpy(), i.cpu().numpy()))
    want_out = np.concatenate([res[0][0], reverse_np(res[1][0], lens, T, np.zeros_like(res[1][0]), SET)], 1)
    want_out[~m] = 0
    assert np.array_equal(out, want_out)
    want_ind = reverse_np(res[1][1], lens, T, res[0][1].copy(), ADD)
    want_ind[~m] = 0
    assert np.array_equal(ind, want_ind)
    assert np.array_equal(bl.get_corr(), np.concatenate([ef.get_corr(), eb.get_corr()]))
    assert np.array_equal(bl.get_params(), np.concatenate([ef.get_params(), eb.get_params()]))
    for e in (bl, ef, eb):
        e.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. the C++ layer (include/klstm_blstm.hpp) agrees with the Python path to the bit
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse,want_id", [(0, 1), (1, 1), (1, 0)], ids=["plain", "fused", "no_in_diff"])
def test_cpp_layer_matches_python(tmp_path, fuse, want_id):
    I, C, R, S, T = 40, 800, 512, 4, 50
    lens = [T, 37, 0, 1]
    pf, pb = rg.trained_params(I, C, R, 7), rg.trained_params(I, C, R, 8)
    x, od = inputs(I, R, T, S, lens, np.random.RandomState(1))
    (tmp_path / "f.bin").write_bytes(kaldi_fmt.binary_model(pf, I, C, R, S))
    (tmp_path / "b.bin").write_bytes(kaldi_fmt.binary_model(pb, I, C, R, S))
    x.tofile(tmp_path / "x.raw")
    od.tofile(tmp_path / "od.raw")
    run("layer", tmp_path / "f.bin", tmp_path / "b.bin", tmp_path / "x.raw", tmp_path / "od.raw", ",".join(map(str, lens)), LR, MOM,
        fuse, want_id, 2, str(tmp_path) + "/")
    bl = k.BidirectionalLstm(I, C, R, S)
    bl.set_params(pf, pb)
    for _ in range(2):
        out, ind = blstm_minibatch(bl, x, od, lens, 2 if fuse else 0, bool(want_id))
    assert np.array_equal(np.fromfile(tmp_path / "out.raw", np.float32).reshape(out.shape), out)
    if want_id:
        assert np.array_equal(np.fromfile(tmp_path / "in_diff.raw", np.float32).reshape(ind.shape), ind)
    assert np.array_equal(np.fromfile(tmp_path / "params.raw", np.float32), bl.get_params())
    bl.close()


def test_cpp_nnet_matches_python(tmp_path):
    """Nnet of Transmit -> BLstm -> Affine -> Softmax with SetSeqLengths against the same chain of Python calls."""
    I, C, R, S, T, P = 40, 800, 512, 4, 40, 96
    lens = [T, 23, 5, 0]
    rng = np.random.RandomState(2)
    pf, pb = rg.trained_params(I, C, R, 9), rg.trained_params(I, C, R, 10)
    W = (0.05 * rng.randn(P, 2 * R)).astype(np.float32)
    b = (0.1 * rng.randn(P)).astype(np.float32)
    x = rng.randn(T * S, I).astype(np.float32)
    od = rng.randn(T * S, P).astype(np.float32)
    od[~pad_mask(lens, T)] = 0
    (tmp_path / "f.bin").write_bytes(kaldi_fmt.binary_model(pf, I, C, R, S))
    (tmp_path / "b.bin").write_bytes(kaldi_fmt.binary_model(pb, I, C, R, S))
    for n, a in (("W", W), ("b", b), ("x", x), ("od", od)):
        a.tofile(tmp_path / (n + ".raw"))
    lr, mom = 1e-3, 0.9
    run("nnet", tmp_path / "f.bin", tmp_path / "b.bin", tmp_path / "W.raw", tmp_path / "b.raw", tmp_path / "x.raw", tmp_path / "od.raw",
        ",".join(map(str, lens)), lr, mom, str(tmp_path) + "/")
    # the Python chain, in Nnet::Propagate / Backpropagate order
    bl = k.BidirectionalLstm(I, C, R, S)
    bl.set_params(pf, pb)
    xd, odd = cuda(x), cuda(od)
    h = torch.empty(T * S, 2 * R, device="cuda")
    a = torch.empty(T * S, P, device="cuda")
    y = torch.empty(T * S, P, device="cuda")
    Wd, bd = cuda(W), cuda(b)
    Wc, bc = torch.zeros_like(Wd), torch.zeros_like(bd)
    torch.cuda.synchronize()
    bl.propagate(xd, lens, h)
    k.affine_propagate(h, Wd, bd, a)
    k.softmax(a, y)
    dh = torch.empty(T * S, 2 * R, device="cuda")
    k.affine_backpropagate(odd, Wd, dh)
    k.affine_update(h, odd, Wd, bd, Wc, bc, lr, lr, mom)
    ind = torch.empty(T * S, I, device="cuda")
    bl.backpropagate(xd, dh, in_diff=ind, momentum=0.9, flags=k.binding.BPTT_FUSE_UPDATE)
    bl.update(lr)
    bl.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(np.fromfile(tmp_path / "out.raw", np.float32).reshape(T * S, P), y.cpu().numpy())
    assert np.array_equal(np.fromfile(tmp_path / "blstm.raw", np.float32), bl.get_params())
    want = np.concatenate([Wd.cpu().numpy().ravel(), bd.cpu().numpy()])
    assert np.array_equal(np.fromfile(tmp_path / "affine.raw", np.float32), want)
    bl.close()
