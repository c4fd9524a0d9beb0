"""The CLDNN front-end kernels on the GPU (the kcnn_* entries of include/klstm_cnn.h) against the two yardsticks of tests/cnn_ref.py.

Convolution: the project's measure, max|gpu - truth64| / max|truth64| per tensor, through margins.bound(); the bar is max(4 x the error of
the float32 twin on the same inputs, FLOOR), FLOOR = 2^-22: the floor tests/test_output_tail_gpu.py uses for the affine products of the
fp32 kernels under this measure (these products are exact f32 products with f32 accumulation on the matrix instruction).  No tolerance
comes from the kernels' own output.  Pooling: bit identity to the twin.  Activations: the cell's forms are documented in klstm_math.h at
<= 3e-7 absolute from the exact functions (hardware exp2 and rcp); their derivatives are two correctly rounded float operations on the
given output: FLOOR under the measure above."""
import numpy as np
import pytest
import torch

from tests import cnn_fmt, cnn_ref
from tests.margins import bound
from tests.test_cnn import run

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
FLOOR = 2.0 ** -22
ACT_ABS = 3e-7
SENTINEL = 12345.0
LAYOUTS = ["contiguous", "padded", "offset"]
SHAPES = [(1, 11, 4, 1), (3, 11, 5, 2), (3, 40, 8, 1), (2, 12, 4, 4)]            # (n, st, pd, ps)
FS = [1, 5, 16, 33, 64]
ROWS = [1, 7, 80, 257, 130]                                                      # 130 and 257: above the gradient's split of 64 rows


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def placed(x, layout):
    """x on the device as `layout` says: (view, whole buffer)"""
    rows, cols = x.shape
    if layout == "contiguous":
        buf = torch.full((rows, cols), SENTINEL, device="cuda")
        view = buf
    else:
        stride = (cols + 1 + 63) // 64 * 64
        buf = torch.full((rows, stride), SENTINEL, device="cuda")
        view = buf[:, 1:cols + 1] if layout == "offset" else buf[:, :cols]
    view.copy_(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)))
    return view, buf


def padding_intact(view, buf, layout):
    if layout == "contiguous":
        return True
    b = buf.cpu().numpy().copy()
    lo = 1 if layout == "offset" else 0
    b[:, lo:lo + view.shape[1]] = SENTINEL
    return bool((b == SENTINEL).all())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def conv_data(rows, n, st, pd, ps, F, seed):
    rng = np.random.RandomState(seed)
    P, K = 1 + (st - pd) // ps, n * pd
    return (rng.randn(rows, n * st).astype(f32), rng.uniform(-0.3, 0.3, (F, K)).astype(f32), rng.uniform(-0.3, 0.3, F).astype(f32),
            rng.randn(rows, P * F).astype(f32))


def check(tag, got, truth, twin):
    err, e32 = cnn_ref.rel_err(got, truth), cnn_ref.rel_err(twin, truth)
    print(f"{tag}: {err:.3g} (twin {e32:.3g}, bar {max(4 * e32, FLOOR):.3g})", flush=True)
    bound(err, max(4 * e32, FLOOR), tag)


def conv_case(rows, n, st, pd, ps, F, layout, other, seed):
    """propagate, backpropagate and gradient of one shape in one layout; the gradient again, and again in the layout `other`"""
    import kaldi_lstm_amd as k
    geom, din = (pd, ps, st), n * st
    x, W, b, od = conv_data(rows, n, st, pd, ps, F, seed)
    tag = f"{rows}x({n},{st},{pd},{ps})xF{F} {layout}"
    Wd, bd = dev(W), dev(b)
    xv, _ = placed(x, layout)
    odv, _ = placed(od, layout)
    outv, outb = placed(np.full_like(od, SENTINEL), layout)
    k.conv_propagate(xv, Wd, bd, outv, geom)
    idv, idb = placed(np.full_like(x, SENTINEL), layout)
    k.conv_backpropagate(odv, Wd, idv, geom)
    fg, bg = torch.full_like(Wd, SENTINEL), torch.full_like(bd, SENTINEL)
    k.conv_gradient(xv, odv, fg, bg, geom)
    fg2, bg2 = torch.full_like(Wd, SENTINEL), torch.full_like(bd, SENTINEL)
    k.conv_gradient(xv, odv, fg2, bg2, geom)
    xo, _ = placed(x, other)
    odo, _ = placed(od, other)
    fg3, bg3 = torch.full_like(Wd, SENTINEL), torch.full_like(bd, SENTINEL)
    k.conv_gradient(xo, odo, fg3, bg3, geom)
    torch.cuda.synchronize()
    assert padding_intact(outv, outb, layout) and padding_intact(idv, idb, layout), f"{tag}: columns from the width up to the stride were written"
    check(f"out {tag}", outv.cpu().numpy(), cnn_ref.conv_forward(x, W, b, geom, f64), cnn_ref.conv_forward(x, W, b, geom, f32))
    check(f"in_diff {tag}", idv.cpu().numpy(), cnn_ref.conv_backward(od, W, geom, din, f64), cnn_ref.conv_backward(od, W, geom, din, f32))
    (fg64, bg64), (fg32, bg32) = cnn_ref.conv_gradient(x, od, geom, F, f64), cnn_ref.conv_gradient(x, od, geom, F, f32)
    check(f"filters_grad {tag}", fg.cpu().numpy(), fg64, fg32)
    check(f"bias_grad {tag}", bg.cpu().numpy(), bg64, bg32)
    assert np.array_equal(bits(fg.cpu().numpy()), bits(fg2.cpu().numpy())) and np.array_equal(bits(bg.cpu().numpy()), bits(bg2.cpu().numpy())), f"{tag}: two runs differ"
    assert np.array_equal(bits(fg.cpu().numpy()), bits(fg3.cpu().numpy())) and np.array_equal(bits(bg.cpu().numpy()), bits(bg3.cpu().numpy())), f"{tag}: the strides change the gradient"


def update_case(rows, n, st, pd, ps, F, layout, seed):
    """kcnn_conv_update over three steps with momentum 0.9, a new input and out_diff at each, against the same recipe in float64 / float32"""
    import kaldi_lstm_amd as k
    geom, lr, lrb, mmt = (pd, ps, st), 0.01, 0.02, 0.9
    _, W, b, _ = conv_data(rows, n, st, pd, ps, F, seed)
    Wd, bd = dev(W), dev(b)
    Wc, bc = torch.zeros_like(Wd), torch.zeros_like(bd)
    ref = {dt: [W.astype(dt), b.astype(dt), np.zeros(W.shape, dt), np.zeros(b.shape, dt)] for dt in (f64, f32)}
    for step in range(3):
        x, _, _, od = conv_data(rows, n, st, pd, ps, F, seed + 1 + step)
        xv, _ = placed(x, layout)
        odv, _ = placed(od, layout)
        k.conv_update(xv, odv, Wd, bd, Wc, bc, lr, lrb, mmt, geom)
        for dt, s in ref.items():
            fg, bg = cnn_ref.conv_gradient(x, od, geom, F, dt)
            s[0], s[2] = cnn_ref.sgd_step(s[0], s[2], fg, lr, mmt, dt)
            s[1], s[3] = cnn_ref.sgd_step(s[1], s[3], bg, lrb, mmt, dt)
    torch.cuda.synchronize()
    tag = f"{rows}x({n},{st},{pd},{ps})xF{F} {layout} after 3 updates"
    for name, got, i in [("filters", Wd, 0), ("bias", bd, 1), ("filters_corr", Wc, 2), ("bias_corr", bc, 3)]:
        check(f"{name} {tag}", got.cpu().numpy(), ref[f64][i], ref[f32][i])


@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("n,st,pd,ps", SHAPES)
def test_convolution_entries_against_float64(n, st, pd, ps, F):
    for i, rows in enumerate(ROWS):
        for j, layout in enumerate(LAYOUTS):
            conv_case(rows, n, st, pd, ps, F, layout, LAYOUTS[(LAYOUTS.index(layout) + 1 + (i + j) % 2) % 3], seed=1000 * i + F)
    update_case(80, n, st, pd, ps, F, LAYOUTS[F % 3], seed=77 + F)


def test_convolution_of_the_440_input_case():
    """(11, 40, 8, 1) with F = 128 at rows = 80: P = 33, K = 88"""
    conv_case(80, 11, 40, 8, 1, 128, "contiguous", "offset", seed=5)
    conv_case(80, 11, 40, 8, 1, 128, "padded", "contiguous", seed=6)
    update_case(80, 11, 40, 8, 1, 128, "contiguous", seed=7)


# Shapes that leave the one-tile plans of klstm_cnn.hip (conv_fwd_plan / conv_bwd_plan, 156 KB of LDS; restated here from the host code):
#   (33, 40, 8, 1) F = 256: D_in = 1320, K = 264.  Forward: 16 rows take 84 KB, so the filters go in 8 tiles of 32 (grid.y = 8, f0 > 0).
#       Backward: 8 rows of accumulator take 42 KB, the filters 4 tiles of 64 (nft = 4: loaded again for every row block and tile).
#       Gradient: grid.y = 8 blocks of 32 f, grid.z = 2 blocks of 256 k, all four waves of z = 0 at work.
#   (60, 40, 8, 1) F = 5: D_in = 2400, K = 480.  Forward: 16 rows (154 KB) do not fit beside a 16-filter tile: RB = 4.
#   (120, 12, 4, 4) F = 4: D_in = 1440, K = 480, P = 3.  Backward: RW0 = 4 rows per wave (184 KB of accumulator) do not fit: RW = 3, RB = 24.
TILED = [(7, 33, 40, 8, 1, 256), (80, 33, 40, 8, 1, 256), (7, 60, 40, 8, 1, 5), (40, 120, 12, 4, 4, 4)]


@pytest.mark.parametrize("rows,n,st,pd,ps,F", TILED)
def test_convolution_on_the_tiled_plans(rows, n, st, pd, ps, F):
    """several filter tiles forward and backward, K > 256 in the gradient, fewer rows per block: the same bar"""
    conv_case(rows, n, st, pd, ps, F, "padded", "contiguous", seed=rows + F)
    conv_case(rows, n, st, pd, ps, F, "offset", "padded", seed=rows + F + 1)
    update_case(rows, n, st, pd, ps, F, "contiguous", seed=rows + F + 2)


def test_in_diff_not_wanted_is_ok():
    import kaldi_lstm_amd as k
    x, W, b, od = conv_data(7, 3, 11, 5, 2, 5, 3)
    odd, Wd = dev(od), dev(W)
    assert k.load_library().kcnn_conv_backpropagate(odd.data_ptr(), odd.stride(0), 7, 33, 20, 5, 2, 11, Wd.data_ptr(), None, 0, None) == 0
    assert k.conv_backpropagate(odd, Wd, None, (5, 2, 11)) is None
    c = k.Convolutional(33, 20, 5, 2, 11, W, b)
    assert c.backward(odd, want=False) is None
    torch.cuda.synchronize()


# ---- pooling: bit identity ----
POOLS = [(5, 3, 3, 1), (33, 16, 3, 3), (33, 128, 3, 3), (7, 5, 2, 2), (4, 1, 4, 1)]          # (Pin, w, z, g); (7, 5, 2, 2): patch 6 lies in no pool


def pool_data(rows, Pin, w, seed):
    """quarters in [-2, 2] (ties everywhere), a row of equal values, and a -0.0 / +0.0 pair in neighbouring patches"""
    rng = np.random.RandomState(seed)
    x = (rng.randint(-8, 9, size=(rows, Pin, w)) / 4.0).astype(f32)
    x[rows // 2] = 0.75
    x[0, 0, :] = -0.0
    if Pin > 1:
        x[0, 1, :] = 0.0
    return x.reshape(rows, Pin * w)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("Pin,w,z,g", POOLS)
def test_pooling_is_the_twin_bit_for_bit(Pin, w, z, g, layout):
    import kaldi_lstm_amd as k
    geom = (z, g, w)
    for rows in (1, 7, 257):
        Q = 1 + (Pin - z) // g
        x = pool_data(rows, Pin, w, rows + Pin)
        od = np.random.RandomState(rows).randn(rows, Q * w).astype(f32)
        want_out = cnn_ref.pool_forward(x, geom)
        want_id = cnn_ref.pool_backward(x, want_out, od, geom)
        xv, _ = placed(x, layout)
        outv, outb = placed(np.full_like(od, SENTINEL), layout)
        k.pool_propagate(xv, outv, geom)
        odv, _ = placed(od, layout)
        idv, idb = placed(np.full_like(x, SENTINEL), layout)
        k.pool_backpropagate(xv, outv, odv, idv, geom)
        torch.cuda.synchronize()
        assert padding_intact(outv, outb, layout) and padding_intact(idv, idb, layout)
        assert np.array_equal(bits(outv.cpu().numpy()), bits(want_out)), f"forward, rows {rows}"
        assert np.array_equal(bits(idv.cpu().numpy()), bits(want_id)), f"backward, rows {rows}"
    if (Pin, w, z, g) == (7, 5, 2, 2):
        assert (want_id.reshape(rows, Pin, w)[:, 6] == 0).all() and not np.signbit(want_id.reshape(rows, Pin, w)[:, 6]).any()


# ---- activations ----
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", [cnn_ref.SIGMOID, cnn_ref.TANH])
def test_activations_against_float64(kind, layout):
    import kaldi_lstm_amd as k
    for rows, cols in [(1, 1), (7, 37), (257, 128)]:
        rng = np.random.RandomState(rows + kind)
        x = (rng.randn(rows, cols) * 3).astype(f32)
        x.reshape(-1)[:2] = [50.0, -50.0][:x.size]
        d = rng.randn(rows, cols).astype(f32)
        xv, _ = placed(x, layout)
        yv, yb = placed(np.full_like(x, SENTINEL), layout)
        k.activation(kind, xv, yv)
        dv, _ = placed(d, layout)
        idv, idb = placed(np.full_like(x, SENTINEL), layout)
        k.activation_diff(kind, yv, dv, idv)
        torch.cuda.synchronize()
        assert padding_intact(yv, yb, layout) and padding_intact(idv, idb, layout)
        y = yv.cpu().numpy()
        name = "sigmoid" if kind == cnn_ref.SIGMOID else "tanh"
        bound(float(np.abs(y.astype(f64) - cnn_ref.activation(kind, x, f64)).max()), ACT_ABS, f"{name} {rows}x{cols} {layout} (absolute)")
        check(f"{name} diff {rows}x{cols} {layout}", idv.cpu().numpy(), cnn_ref.activation_diff(kind, y, d, f64), cnn_ref.activation_diff(kind, y, d, f32))


# ---- the Python classes, once ----
def test_python_classes_against_the_twins():
    import kaldi_lstm_amd as k
    n, st, pd, ps, F, rows = 3, 16, 4, 1, 8, 40
    geom, P = (pd, ps, st), 13
    x, W, b, _ = conv_data(rows, n, st, pd, ps, F, 11)
    conv, pool, act = k.Convolutional(n * st, P * F, pd, ps, st, W, b), k.MaxPooling(P * F, 4 * F, 3, 3, F), k.Sigmoid()
    xd = dev(x)
    h1 = conv.forward(xd)
    h2 = pool.forward(h1)
    y = act.forward(h2)
    od = np.random.RandomState(12).randn(rows, 4 * F).astype(f32)
    d2 = act.backward(y, dev(od))
    d1 = pool.backward(h1, h2, d2)
    d0 = conv.backward(d1)
    fg, bg = conv.gradient(xd, d1)
    conv.update(xd, d1, 0.05, momentum=0.0)
    torch.cuda.synchronize()
    h1n, yn, d2n, d1n = h1.cpu().numpy(), y.cpu().numpy(), d2.cpu().numpy(), d1.cpu().numpy()
    check("Convolutional.forward", h1n, cnn_ref.conv_forward(x, W, b, geom, f64), cnn_ref.conv_forward(x, W, b, geom, f32))
    assert np.array_equal(bits(h2.cpu().numpy()), bits(cnn_ref.pool_forward(h1n, (3, 3, F))))
    bound(float(np.abs(yn.astype(f64) - cnn_ref.activation(cnn_ref.SIGMOID, h2.cpu().numpy(), f64)).max()), ACT_ABS, "Sigmoid.forward (absolute)")
    check("Sigmoid.backward", d2n, cnn_ref.activation_diff(cnn_ref.SIGMOID, yn, od, f64), cnn_ref.activation_diff(cnn_ref.SIGMOID, yn, od, f32))
    assert np.array_equal(bits(d1n), bits(cnn_ref.pool_backward(h1n, h2.cpu().numpy(), d2n, (3, 3, F))))
    check("Convolutional.backward", d0.cpu().numpy(), cnn_ref.conv_backward(d1n, W, geom, n * st, f64), cnn_ref.conv_backward(d1n, W, geom, n * st, f32))
    (fg64, bg64), (fg32, bg32) = cnn_ref.conv_gradient(x, d1n, geom, F, f64), cnn_ref.conv_gradient(x, d1n, geom, F, f32)
    check("Convolutional.gradient filters", fg.cpu().numpy(), fg64, fg32)
    check("Convolutional.gradient bias", bg.cpu().numpy(), bg64, bg32)
    check("Convolutional.update filters", conv.filters.cpu().numpy(), W.astype(f64) - 0.05 * fg64, W - f32(0.05) * fg32)
    check("Convolutional.update bias", conv.bias.cpu().numpy(), b.astype(f64) - 0.05 * bg64, b - f32(0.05) * bg32)


# ---- the C++ layers through Nnet::Propagate / Backpropagate ----
def front_end_chain(x, W, b, od, geom, pool, steps, lr, mmt, dt):
    """<ConvolutionalComponent> <MaxPoolingComponent> as Nnet::Backpropagate drives them (last component first: backpropagate, then
    update); returns [(out, in_diff)] of every step and the trained filters and bias"""
    F = W.shape[0]
    W, b = W.astype(dt), b.astype(dt)
    Wc, bc = np.zeros_like(W), np.zeros_like(b)
    dumps = []
    for _ in range(steps):
        h1 = cnn_ref.conv_forward(x, W, b, geom, dt)
        h2 = cnn_ref.pool_forward(h1, pool)
        d1 = cnn_ref.pool_backward(h1, h2, od.astype(dt), pool)
        d0 = cnn_ref.conv_backward(d1, W, geom, x.shape[1], dt)
        fg, bg = cnn_ref.conv_gradient(x, d1, geom, F, dt)
        W, Wc = cnn_ref.sgd_step(W, Wc, fg, lr, mmt, dt)
        b, bc = cnn_ref.sgd_step(b, bc, bg, lr, mmt, dt)
        dumps.append((h2, d0))
    return dumps, W, b


def test_cpp_convolution_and_pooling_layers_through_nnet(tmp_path):
    """tests/cpp/cnn_test.cpp layers: three steps of Nnet::Propagate / Backpropagate (with Update) at lr 0.02 and momentum 0.9 on 3 x 16
    inputs, patches of 4, 8 filters, pools 3 / 3: out and the first component's in_diff of every step and the trained filters and bias
    against the float64 chain, the bar from the float32 chain"""
    n, st, pd, ps, F, z, g, rows, steps, lr, mmt = 3, 16, 4, 1, 8, 3, 3, 70, 3, 0.02, 0.9
    P, Q, geom, pool = 13, 4, (pd, ps, st), (z, g, F)
    x, W, b, _ = conv_data(rows, n, st, pd, ps, F, 21)
    od = np.random.RandomState(22).randn(rows, Q * F).astype(f32)
    layers = [("conv", W, b, n * st, P * F, pd, ps, st), ("pool", P * F, Q * F, z, g, F)]
    model = cnn_fmt.nnet_binary(layers)
    (tmp_path / "n.bin").write_bytes(model)
    x.tofile(tmp_path / "x.raw"); od.tofile(tmp_path / "od.raw")
    run("layers", tmp_path / "n.bin", tmp_path / "x.raw", tmp_path / "od.raw", rows, lr, mmt, steps, tmp_path / "dump.raw", tmp_path / "out.bin")
    dump = np.fromfile(tmp_path / "dump.raw", dtype=f32).reshape(steps, -1)
    d64, W64, b64 = front_end_chain(x, W, b, od, geom, pool, steps, lr, mmt, f64)
    d32, W32, b32 = front_end_chain(x, W, b, od, geom, pool, steps, lr, mmt, f32)
    for s in range(steps):
        check(f"out, step {s}", dump[s, :rows * Q * F].reshape(rows, Q * F), d64[s][0], d32[s][0])
        check(f"in_diff, step {s}", dump[s, rows * Q * F:].reshape(rows, n * st), d64[s][1], d32[s][1])
    out = (tmp_path / "out.bin").read_bytes()
    assert len(out) == len(model)
    at = model.index(b"<Filters> ") + len(b"<Filters> FM ") + 10                    # behind the two int32 of the matrix header
    check("trained filters", np.frombuffer(out[at:at + 4 * W.size], dtype="<f4").reshape(W.shape), W64, W32)
    at = model.index(b"<Bias> ") + len(b"<Bias> FV ") + 5
    check("trained bias", np.frombuffer(out[at:at + 4 * b.size], dtype="<f4"), b64, b32)


@pytest.mark.parametrize("name,kind", [("sigmoid", cnn_ref.SIGMOID), ("tanh", cnn_ref.TANH)])
def test_cpp_activation_layers_through_nnet(tmp_path, name, kind):
    """a net of <Tanh> <Sigmoid> (or the other way round) against the exact composition in float64, with bars that follow from the
    documented 3e-7 of each function (worked out at the assertions)"""
    rows, dim = 33, 24
    x = (np.random.RandomState(31).randn(rows, dim) * 2).astype(f32)
    od = np.random.RandomState(32).randn(rows, dim).astype(f32)
    other = "tanh" if name == "sigmoid" else "sigmoid"
    (tmp_path / "n.bin").write_bytes(cnn_fmt.nnet_binary([(name, dim), (other, dim)]))
    x.tofile(tmp_path / "x.raw"); od.tofile(tmp_path / "od.raw")
    run("layers", tmp_path / "n.bin", tmp_path / "x.raw", tmp_path / "od.raw", rows, 0.1, 0.0, 1, tmp_path / "dump.raw", tmp_path / "out.bin")
    dump = np.fromfile(tmp_path / "dump.raw", dtype=f32)
    y, d0 = dump[:rows * dim].reshape(rows, dim), dump[rows * dim:].reshape(rows, dim)
    h64 = cnn_ref.activation(kind, x, f64)
    y64 = cnn_ref.activation(1 - kind, h64, f64)
    # the second activation's slope is at most 1 (tanh) or 1/4 (sigmoid): the first one's deviation passes at most undiminished
    bound(float(np.abs(y - y64).max()), 2 * ACT_ABS, f"{name} -> {other} out (absolute)")
    d64 = cnn_ref.activation_diff(kind, h64, cnn_ref.activation_diff(1 - kind, y64, od, f64), f64)
    # a derivative factor, y (1 - y) or 1 - y y, has a slope of at most 2 in y: the second moves by <= 2 x (2 x 3e-7), the first by
    # <= 2 x 3e-7, both factors are below 1: 6 x 3e-7 <= 8 x 3e-7, and four float roundings
    bound(float(np.abs(d0 - d64).max()), (8 * ACT_ABS + 4 * 2.0 ** -24) * float(np.abs(od).max()), f"{name} -> {other} in_diff (absolute)")


# ---- the whole CLDNN under the trainers and the decoder ----
def test_cldnn_under_train_lstm_streams_ctc_training_and_the_greedy_decoder(tmp_path):
    """<ConvolutionalComponent> <MaxPoolingComponent> <Sigmoid> <AffineTransform> <LstmProjectedStreams> <AffineTransform> <Softmax>: 3 x 16
    inputs, patches of 4 every 1, 8 filters, pools 3 / 3, an affine to 24, an LSTM 24 -> 32 / 16, 20 pdfs, through tests/cpp/cnn_test.cpp
    train: five minibatches of TrainLstmStreams (S = 4, T = 20, momentum 0.9), then one minibatch of TrainCtcWholeUtterances, then
    that minibatch through CtcGreedyDecoder.  Every parameter tensor after the stream minibatches and after the CTC minibatch against
    the float64 run of tests/test_cnn.py cldnn_train (cnn_ref + oracle/components.py + the LSTM oracle + torch's ctc_loss); the bar is
    4 x the error of the float32 run of the same loop, floored at 2^-22.  The decoder's frame classes are the float32 run's arg-max
    on every row whose float64 top-two margin exceeds that run's error; at most 5 % of the valid rows may be left out (the seed keeps the
    twin alone under that: tests/test_cnn.py), and a stream all of whose rows are decided has the twin's collapsed path as hypothesis."""
    from tests import kaldi_fmt
    from tests.test_cnn import C, HID, R, TRAIN, cldnn_ctc_utts, cldnn_net, cldnn_train, cldnn_utts, decided_rows
    from tests.test_component import _pack_utts
    layers, utts, cu = cldnn_net(), cldnn_utts(), cldnn_ctc_utts()
    (tmp_path / "n.bin").write_bytes(cnn_fmt.nnet_binary(layers))
    _pack_utts(utts).tofile(tmp_path / "u.raw")
    _pack_utts(cu).tofile(tmp_path / "c.raw")
    files = [tmp_path / n for n in ("before.raw", "streams.raw", "ctc.raw", "classes.raw")]
    line = run("train", tmp_path / "n.bin", tmp_path / "u.raw", tmp_path / "c.raw", TRAIN["S"], TRAIN["T"], TRAIN["delay"], TRAIN["lr"],
               TRAIN["mmt"], *files).stdout
    head = line.split("|")[0].split()
    nb, s64, _ = cldnn_train(layers, utts, f64, **TRAIN)
    _, s32, _ = cldnn_train(layers, utts, f32, **TRAIN)
    _, c64, (y64, lens) = cldnn_train(layers, utts, f64, ctc_utts=cu, **TRAIN)
    _, c32, (y32, _) = cldnn_train(layers, utts, f32, ctc_utts=cu, **TRAIN)
    T, S = y64.shape[:2]
    assert head[0] == "OK" and int(head[1]) == len(utts) and int(head[2]) == nb == 5
    assert int(head[3]) == len(cu) and int(head[4]) == 1 and float(head[5]) == 0 and int(head[6]) == T
    # the order of the dump is the order of the reference's tensors: the untrained dump is the model's own numbers, bit for bit
    start = [layers[0][1], layers[0][2], layers[3][1], layers[3][2]] + kaldi_fmt.parts(layers[4][1], HID, C, R) + [layers[5][1], layers[5][2]]
    assert np.array_equal(bits(np.fromfile(files[0], dtype=f32)), bits(np.concatenate([a.reshape(-1) for a in start])))
    for what, path, p64, p32 in [(f"after {nb} stream minibatches", files[1], s64, s32), ("after the CTC minibatch", files[2], c64, c32)]:
        got, at = np.fromfile(path, dtype=f32), 0
        for (name, t64), a0 in zip(p64.items(), start):
            assert t64.shape == a0.shape
            check(f"{name} {what}", got[at:at + a0.size].reshape(a0.shape), t64, p32[name])
            at += a0.size
        assert at == got.size
    decided, path, err = decided_rows(y64, y32, lens)
    valid = int(sum(lens))
    classes = np.fromfile(files[3], dtype=np.int32).reshape(T, S)
    print(f"decoder: twin's error on the posteriors {err:.3g}, {valid - int(decided.sum())} of {valid} valid rows left out", flush=True)
    assert valid - int(decided.sum()) <= 0.05 * valid
    assert np.array_equal(classes[decided], path[decided])
    assert (classes[np.arange(T)[:, None] >= np.asarray(lens)[None, :]] == -1).all()          # padding rows
    hyps = [[int(c) for c in h.split()] for h in line.strip().split("|")[1:]]
    assert len(hyps) == S
    for s_ in range(S):
        if decided[:lens[s_], s_].all():
            p = path[:lens[s_], s_]
            assert hyps[s_] == [int(c) for i, c in enumerate(p) if c != 0 and (i == 0 or c != p[i - 1])], s_
