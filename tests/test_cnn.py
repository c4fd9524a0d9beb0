"""The CLDNN front-end components without a GPU (include/klstm_cnn.h; <ConvolutionalComponent>, <MaxPoolingComponent>, <Sigmoid>, <Tanh>
of include/klstm_nnet.hpp): the numpy yardsticks of tests/cnn_ref.py pinned against torch's conv1d / max_pool1d with autograd in float64,
the overlap rule of the pooling twin on a case computed by hand, kcnn_conv_plan and every argument refusal of the entries, the exported
names, and model files with the four components in them, text and binary."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import cnn_fmt, cnn_ref, cpp_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ("klstm.h", "klstm_cnn.h", "klstm_dropout.h", "klstm_component.hpp", "klstm_kaldi_io.hpp", "klstm_trainer.hpp", "klstm_nnet.hpp")
NAMES = ["kcnn_activation", "kcnn_activation_diff", "kcnn_conv_backpropagate", "kcnn_conv_gradient", "kcnn_conv_plan", "kcnn_conv_propagate",
         "kcnn_conv_update", "kcnn_conv_workspace_floats", "kcnn_pool_backpropagate", "kcnn_pool_propagate"]


def build_cnn_driver():
    return cpp_driver.build("cnn_test", headers=HEADERS)


def run(*args, ok=True):
    return cpp_driver.run("cnn_test", *args, ok=ok, headers=HEADERS)


# ---- the yardsticks against torch ----
CONV_SHAPES = [(1, 11, 4, 1), (3, 11, 5, 2), (3, 40, 8, 1), (2, 12, 4, 4)]          # (n, st, pd, ps)


@pytest.mark.parametrize("n,st,pd,ps", CONV_SHAPES)
@pytest.mark.parametrize("F", [1, 5])
def test_convolution_yardstick_is_torch_conv1d(n, st, pd, ps, F):
    """channels = n, length = st, kernel pd, stride ps; conv1d gives [rows, F, P]: transposed to patch-major"""
    rng = np.random.RandomState(n * 100 + st + F)
    rows, P, K = 7, 1 + (st - pd) // ps, n * pd
    x, W, b = rng.randn(rows, n * st), rng.uniform(-0.3, 0.3, (F, K)), rng.randn(F)
    od = rng.randn(rows, P * F)
    assert cnn_ref.conv_numbers(n * st, P * F, pd, ps, st) == (n, P, K, F)
    tx = torch.tensor(x.reshape(rows, n, st), requires_grad=True)
    tW = torch.tensor(W.reshape(F, n, pd), requires_grad=True)
    tb = torch.tensor(b, requires_grad=True)
    ty = torch.nn.functional.conv1d(tx, tW, tb, stride=ps).transpose(1, 2).reshape(rows, P * F)
    ty.backward(torch.tensor(od))
    geom = (pd, ps, st)
    out = cnn_ref.conv_forward(x, W, b, geom, np.float64)
    ind = cnn_ref.conv_backward(od, W, geom, n * st, np.float64)
    fg, bg = cnn_ref.conv_gradient(x, od, geom, F, np.float64)
    for name, got, want in [("out", out, ty.detach().numpy()), ("in_diff", ind, tx.grad.numpy().reshape(rows, n * st)),
                            ("filters_grad", fg, tW.grad.numpy().reshape(F, K)), ("bias_grad", bg, tb.grad.numpy())]:
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), name
    # the float32 run of the same recipe is near it
    assert cnn_ref.rel_err(cnn_ref.conv_forward(x.astype(np.float32), W.astype(np.float32), b.astype(np.float32), geom, np.float32), out) < 1e-5


@pytest.mark.parametrize("Pin,w,z", [(6, 3, 3), (33, 16, 3), (8, 5, 2)])
def test_pooling_yardstick_is_torch_max_pool1d_without_overlap_or_ties(Pin, w, z):
    rng = np.random.RandomState(Pin + w)
    rows, g = 5, z
    Pin = Pin // z * z
    Q = Pin // z
    x = rng.permutation(rows * Pin * w).reshape(rows, Pin * w).astype(np.float64)          # tie-free
    od = rng.randn(rows, Q * w)
    tx = torch.tensor(x.reshape(rows, Pin, w).transpose(0, 2, 1).copy(), requires_grad=True)      # [rows, w, Pin]: pooled along the patches
    ty = torch.nn.functional.max_pool1d(tx, z, g)
    want_out = ty.detach().numpy().transpose(0, 2, 1).reshape(rows, Q * w)
    ty.backward(torch.tensor(od.reshape(rows, Q, w).transpose(0, 2, 1).copy()))
    out = cnn_ref.pool_forward(x, (z, g, w))
    assert np.array_equal(out, want_out)
    ind = cnn_ref.pool_backward(x, out, od, (z, g, w))
    assert np.array_equal(ind, tx.grad.numpy().transpose(0, 2, 1).reshape(rows, Pin * w))


def test_pooling_overlap_rule_on_a_hand_computed_case():
    """z = 3, g = 1, five patches of one value: pools {0,1,2}, {1,2,3}, {2,3,4}; c = 1, 2, 3, 2, 1.
    x = 1 5 5 2 5: maxima 5 5 5.  out_diff = 1 10 100.
      p0 (pool 0): 1 != 5                      -> 0
      p1 (pools 0, 1): tie in both: (1 + 10)/2 -> 5.5
      p2 (pools 0, 1, 2): (1 + 10 + 100) / 3   -> 111 * fl(1/3)
      p3 (pools 1, 2): 2 != 5                  -> 0
      p4 (pool 2): 100 / 1                     -> 100
    Tied inputs each receive the whole diff; the factor 1 / c_p is one float division, applied last."""
    f32 = np.float32
    x = np.array([[1, 5, 5, 2, 5]], f32)
    out = cnn_ref.pool_forward(x, (3, 1, 1))
    assert np.array_equal(out, np.array([[5, 5, 5]], f32))
    ind = cnn_ref.pool_backward(x, out, np.array([[1, 10, 100]], f32), (3, 1, 1))
    want = np.array([[0, f32(11) * (f32(1) / f32(2)), f32(111) * (f32(1) / f32(3)), 0, 100]], f32)
    assert np.array_equal(ind.view(np.uint32), want.view(np.uint32))
    # a patch that no pool contains gets +0.0: 5 patches, z = 2, g = 3 leaves patch 2 out; 6 patches (Q rounds down) patch 5 as well
    assert cnn_ref.pool_numbers(5, 2, 2, 3, 1) == (5, 2) and cnn_ref.pool_numbers(6, 2, 2, 3, 1) == (6, 2) and cnn_ref.pool_numbers(6, 3, 2, 3, 1) is None
    x = np.array([[3, 1, 9, 2, 4, 8]], f32)
    out = cnn_ref.pool_forward(x, (2, 3, 1))
    ind = cnn_ref.pool_backward(x, out, np.array([[-1, -2]], f32), (2, 3, 1))
    assert np.array_equal(out, np.array([[3, 4]], f32))
    assert np.array_equal(ind.view(np.uint32), np.array([[-1, 0, 0, 0, -2, 0]], f32).view(np.uint32))
    # -0.0 and +0.0 compare equal: both receive the diff
    x = np.array([[-0.0, 0.0, -1.0]], f32)
    out = cnn_ref.pool_forward(x, (3, 1, 1))
    assert np.array_equal(out.view(np.uint32), np.array([[-0.0]], f32).view(np.uint32))            # the first stays: +0.0 > -0.0 is false
    assert np.array_equal(cnn_ref.pool_backward(x, out, np.array([[2]], f32), (3, 1, 1)), np.array([[2, 2, 0]], f32))


def test_activation_yardsticks():
    x = np.array([[-50, -1, 0, 0.5, 50]], np.float32)
    y = cnn_ref.activation(cnn_ref.SIGMOID, x, np.float64)
    assert np.allclose(y, torch.sigmoid(torch.tensor(x, dtype=torch.float64)).numpy(), rtol=1e-14, atol=0)
    t = cnn_ref.activation(cnn_ref.TANH, x, np.float64)
    assert np.allclose(t, np.tanh(x.astype(np.float64)))
    d = np.ones_like(x)
    assert np.allclose(cnn_ref.activation_diff(cnn_ref.SIGMOID, y, d, np.float64), y * (1 - y))
    assert np.allclose(cnn_ref.activation_diff(cnn_ref.TANH, t, d, np.float64), 1 - t * t)


# ---- the entries (host side) ----
def test_conv_plan_is_the_yardsticks_numbers():
    import kaldi_lstm_amd as k
    for n, st, pd, ps in CONV_SHAPES + [(11, 40, 8, 1)]:
        for F in (1, 5, 128):
            P = 1 + (st - pd) // ps
            assert k.conv_plan(n * st, P * F, pd, ps, st) == cnn_ref.conv_numbers(n * st, P * F, pd, ps, st) == (n, P, n * pd, F)
    for bad in [(12, 6, 4, 4, 5), (12, 6, 13, 1, 12), (12, 6, 4, 3, 12), (12, 7, 4, 4, 12), (12, 6, 0, 4, 12), (-12, 6, 4, 4, 12)]:
        assert cnn_ref.conv_numbers(*bad) is None
        with pytest.raises(k.KlstmError) as ei:
            k.conv_plan(*bad)
        assert ei.value.status == 1 and "kcnn_conv_plan: " in str(ei.value)


def test_every_refusal_answers_before_any_hip_call():
    """tests/cpp/cnn_test.cpp errors: every KLSTM_ERR_ARG case of the ten entries with host pointers that are never followed and no
    device in the machine, each with its message; zero rows and a null in_diff are KLSTM_OK"""
    out = run("errors").stdout
    assert out.startswith("OK 49 refusals"), out


def test_refusals_through_the_python_declarations():
    """the eight device entries through binding.py's argtypes with pointer values that are never followed: a wrong declaration on an
    error path shows here.  Also the capacity refusals: shapes whose smallest tiling does not fit LDS."""
    import kaldi_lstm_amd as k
    lib, A, B, C, D = k.load_library(), 0x1000, 0x2000, 0x3000, 0x4000
    g = (12, 6, 4, 4, 12)                                   # in, out, pd, ps, st: P = 3, K = 4, F = 2
    cases = [
        (lambda: lib.kcnn_conv_propagate(A, 12, 2, 12, 7, 4, 4, 12, B, C, D, 6, None), "kcnn_conv_propagate: inconsistent numbers"),
        (lambda: lib.kcnn_conv_propagate(A, 12, 2, *g, B, C, D, 5, None), "kcnn_conv_propagate: row stride"),
        (lambda: lib.kcnn_conv_propagate(A, 12, 2, *g, None, C, D, 6, None), "kcnn_conv_propagate: null argument"),
        (lambda: lib.kcnn_conv_backpropagate(A, 5, 2, *g, B, D, 12, None), "kcnn_conv_backpropagate: row stride"),
        (lambda: lib.kcnn_conv_backpropagate(A, 6, -1, *g, B, D, 12, None), "kcnn_conv_backpropagate: rows"),
        (lambda: lib.kcnn_conv_gradient(A, 12, B, 6, 2, *g, C, D, D, 11, None), "kcnn_conv_gradient: workspace of 11 floats, 12 needed"),
        (lambda: lib.kcnn_conv_gradient(A, 11, B, 6, 2, *g, C, D, D, 64, None), "kcnn_conv_gradient: row stride"),
        (lambda: lib.kcnn_conv_update(A, 12, B, 6, 2, *g, C, D, C, None, 0.1, 0.1, 0.9, D, 64, None), "kcnn_conv_update: null argument"),
        (lambda: lib.kcnn_conv_update(A, 12, B, 6, 2, *g, C, D, C, D, 0.1, 0.1, 0.9, D, 3, None), "kcnn_conv_update: workspace of 3 floats"),
        (lambda: lib.kcnn_pool_propagate(A, 15, 2, 15, 6, 3, 1, 3, B, 9, None), "kcnn_pool_propagate: inconsistent numbers"),
        (lambda: lib.kcnn_pool_propagate(A, 14, 2, 15, 9, 3, 1, 3, B, 9, None), "kcnn_pool_propagate: row stride"),
        (lambda: lib.kcnn_pool_backpropagate(A, 15, B, 9, C, 8, 2, 15, 9, 3, 1, 3, D, 15, None), "kcnn_pool_backpropagate: row stride"),
        (lambda: lib.kcnn_pool_backpropagate(A, 15, None, 9, C, 9, 2, 15, 9, 3, 1, 3, D, 15, None), "kcnn_pool_backpropagate: null argument"),
        (lambda: lib.kcnn_activation(2, A, 8, 2, 8, B, 8, None), "kcnn_activation: unknown kind"),
        (lambda: lib.kcnn_activation(1, A, 8, 2, 8, A, 16, None), "kcnn_activation: in == out with two strides"),
        (lambda: lib.kcnn_activation_diff(0, A, 8, B, 8, 2, 8, C, 7, None), "kcnn_activation_diff: row stride"),
        (lambda: lib.kcnn_activation_diff(0, A, 8, B, 8, 2, -8, C, 8, None), "kcnn_activation_diff: bad size"),
        # capacity: K = 2400 (300 blocks of 8, one patch): 16 filters alone take 154 KB of the forward kernel's LDS, 4 of the backward's
        # 38 KB beside the table and a row -- the forward call is refused; an input row of 8000 floats is beyond the gradient's 16-row stage
        (lambda: lib.kcnn_conv_propagate(A, 2400, 2, 2400, 5, 8, 1, 8, B, C, D, 5, None), "kcnn_conv_propagate: K = 2400, D_in = 2400 do not fit"),
        (lambda: lib.kcnn_conv_gradient(A, 8000, B, 33, 2, 8000, 33, 8, 1, 40, C, D, D, 10 ** 9, None), "kcnn_conv_gradient: an input row of 8000 floats does not fit"),
        (lambda: lib.kcnn_conv_backpropagate(A, 5, 2, 40000, 5, 8, 1, 8, B, D, 40000, None), "kcnn_conv_backpropagate: K = 40000, D_in = 40000 do not fit")]
    for call, msg in cases:
        assert call() == 1 and msg in lib.klstm_last_error().decode(), msg
    # zero rows and an unwanted in_diff through the same declarations
    assert lib.kcnn_conv_propagate(None, 0, 0, *g, None, None, None, 0, None) == 0 and lib.kcnn_conv_backpropagate(A, 6, 2, *g, B, None, 0, None) == 0
    assert lib.kcnn_activation_diff(0, A, 8, B, 8, 2, 8, None, 0, None) == 0 and lib.kcnn_pool_backpropagate(A, 15, B, 9, C, 9, 2, 15, 9, 3, 1, 3, None, 0, None) == 0


def test_exported_kcnn_names_are_the_header_s_and_klstm_names_are_unchanged():
    import kaldi_lstm_amd as k
    out = subprocess.run(["nm", "-D", "--defined-only", k.lib_path()], capture_output=True, text=True, check=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    assert sorted(s for s in syms if s.startswith("kcnn_")) == NAMES
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "klstm_cnn.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(kcnn_[a-z_0-9]+)\s*\(", hdr))) == NAMES
    assert "kcnn_" not in open(os.path.join(ROOT, "include", "klstm.h")).read()          # a family of its own, like kdrop_* and knlm_*
    want = open(os.path.join(ROOT, "tests", "golden", "klstm_abi_names.txt")).read().split()
    assert sorted(s for s in syms if s.startswith("klstm_")) == want


# ---- model files (host only) ----
N_BLOCKS, ST, PD, PS, F, POOL, HID, C, R, NPDF, S = 3, 16, 4, 1, 8, 3, 24, 32, 16, 20, 4


def dyadic(shape, seed):
    """multiples of 1/8 in [-1, 1]: the same digits in %.9g and in a stream's six"""
    return (np.random.RandomState(seed).randint(-8, 9, size=shape) / 8.0).astype(np.float32)


def make_layers(pd=PD):
    """<ConvolutionalComponent> <MaxPoolingComponent> <Sigmoid> <AffineTransform> <LstmProjectedStreams> <AffineTransform> <Softmax>:
    3 x 16 inputs, patches of 4 every 1 (13 patches, the last in no pool; 12 with pd = 5), 8 filters, pools of 3 every 3 (4 pools),
    affine to 24, LSTM 24 -> 32 -> 16, 20 pdfs"""
    P_ = 1 + (ST - pd) // PS
    g = POOL
    Q_ = 1 + (P_ - POOL) // g
    nparams = 4 * C * HID + 4 * C * R + 4 * C + 3 * C + R * C
    return [("conv", dyadic((F, N_BLOCKS * pd), 1), dyadic(F, 2), N_BLOCKS * ST, P_ * F, pd, PS, ST), ("pool", P_ * F, Q_ * F, POOL, g, F),
            ("sigmoid", Q_ * F), ("affine", dyadic((HID, Q_ * F), 3), dyadic(HID, 4)), ("lstm_streams", dyadic(nparams, 5), HID, C, R, S),
            ("affine", dyadic((NPDF, R), 6), dyadic(NPDF, 7)), ("softmax", NPDF)]


MARKERS = ["<ConvolutionalComponent>", "<MaxPoolingComponent>", "<Sigmoid>", "<AffineTransform>", "<LstmProjectedStreams>", "<AffineTransform>", "<Softmax>"]


@pytest.mark.parametrize("pd", [4, 5])
def test_model_with_the_front_end_roundtrips_text_binary_text(tmp_path, pd):
    """fails without the feature: Unknown component marker <ConvolutionalComponent>"""
    layers = make_layers(pd)
    text, binary = cnn_fmt.nnet_text(layers), cnn_fmt.nnet_binary(layers)
    if pd == 5:
        assert b"\n<ConvolutionalComponent> 96 48 <PatchDim> 5 <PatchStep> 1 <PatchStride> 16 <LearnRateCoef> 1 <BiasLearnRateCoef> 1 <MaxNorm> 0 <Filters>  [\n" in text
        assert b"]\n<Bias>  [ " in text and b"\n<MaxPoolingComponent> 32 96 <PoolSize> 3 <PoolStep> 3 <PoolStride> 8 \n<Sigmoid> 32 32 \n" in text
        assert b"<MaxPoolingComponent> \x04\x20\x00\x00\x00\x04\x60\x00\x00\x00<PoolSize> \x04\x03\x00\x00\x00<PoolStep> \x04\x03\x00\x00\x00<PoolStride> \x04\x08\x00\x00\x00<Sigmoid> " in binary
    (tmp_path / "n.txt").write_bytes(text)
    out = run("nnet_copy", tmp_path / "n.txt", 1, tmp_path / "n.bin").stdout.split()
    nparams = sum(int(np.prod(a.shape)) for l in layers for a in l[1:3] if isinstance(a, np.ndarray) and l[0] != "lstm_streams") + layers[4][1].size
    assert out == ["OK", "7", str(nparams)] + MARKERS
    assert (tmp_path / "n.bin").read_bytes() == binary
    run("nnet_copy", tmp_path / "n.bin", 0, tmp_path / "n2.txt")
    assert (tmp_path / "n2.txt").read_bytes() == text
    run("nnet_copy", tmp_path / "n2.txt", 1, tmp_path / "n2.bin")
    assert (tmp_path / "n2.bin").read_bytes() == binary


def test_tokens_before_filters_are_read_in_any_order_and_tanh_is_a_component(tmp_path):
    layers = make_layers(5)
    layers[2] = ("tanh", layers[2][1])
    other = ["<MaxNorm>", "<PatchStride>", "<BiasLearnRateCoef>", "<PatchDim>", "<LearnRateCoef>", "<PatchStep>"]
    (tmp_path / "n.txt").write_bytes(cnn_fmt.nnet_text(layers, conv_token_order=other))
    out = run("nnet_copy", tmp_path / "n.txt", 0, tmp_path / "n2.txt").stdout.split()
    assert out[3:] == MARKERS[:2] + ["<Tanh>"] + MARKERS[3:]
    assert (tmp_path / "n2.txt").read_bytes() == cnn_fmt.nnet_text(layers)                 # written in the one order


CONV = "<ConvolutionalComponent> 6 12 <PatchDim> 4 <PatchStep> 4 <PatchStride> 12 <Filters>  [\n  1 2 3 4 \n  5 6 7 8 ]\n<Bias>  [ 1 2 ]\n"


@pytest.mark.parametrize("body,why", [
    (CONV.replace("<PatchStride> 12", "<PatchStride> 5"), "does not divide the input dim"),
    (CONV.replace("<PatchDim> 4", "<PatchDim> 13"), "above the patch stride"),
    (CONV.replace("<PatchStep> 4", "<PatchStep> 3"), "does not divide stride - dim"),
    (CONV.replace(" 6 12 ", " 7 12 "), "do not divide the output dim"),
    (CONV.replace("<PatchStep> 4 ", ""), "a number below 1"),
    (CONV.replace("  5 6 7 8 ]", "  5 6 7 8 \n  9 9 9 9 ]"), "<Filters> 3 x 4"),
    (CONV.replace("[ 1 2 ]", "[ 1 2 3 ]"), "<Bias> 3"),
    (CONV.replace("<PatchDim> 4", "<PatchSize> 4"), "unknown token <PatchSize>"),
    (CONV.replace("<Bias>", "<Biases>"), "<Bias>"),
    (CONV + "<MaxPoolingComponent> 2 6 <PoolSize> 3 <PoolStep> 1 <PoolStride> 4 \n", "MaxPoolingComponent: inconsistent numbers"),
    (CONV + "<MaxPoolingComponent> 4 6 <PoolSize> 3 <PoolStep> 1 <PoolStride> 2 \n", "MaxPoolingComponent: inconsistent numbers"),
    (CONV + "<MaxPoolingComponent> 2 6 <PoolStep> 1 <PoolSize> 3 <PoolStride> 2 \n", "<PoolSize>"),
    (CONV + "<Sigmoid> 6 5 \n", "<Sigmoid>: input dim"),
    (CONV + "<Tanh> 5 6 \n", "<Tanh>: input dim")])
def test_inconsistent_components_are_refused(tmp_path, body, why):
    (tmp_path / "n.txt").write_bytes(b"<Nnet> \n" + body.encode() + b"</Nnet> \n")
    r = run("nnet_copy", tmp_path / "n.txt", 1, tmp_path / "n.bin", ok=False)
    assert r.returncode == 3 and r.stdout.startswith("EXCEPTION:") and why in r.stdout, r.stdout


def test_the_consistent_form_of_that_component_is_accepted(tmp_path):
    (tmp_path / "n.txt").write_bytes(b"<Nnet> \n" + CONV.encode() + b"<MaxPoolingComponent> 2 6 <PoolSize> 3 <PoolStep> 1 <PoolStride> 2 \n<Tanh> 2 2 \n</Nnet> \n")
    assert run("nnet_copy", tmp_path / "n.txt", 1, tmp_path / "n.bin").stdout.split()[:3] == ["OK", "3", "10"]


# ---- the whole CLDNN in a trainer: the reference run (tests/test_cnn_gpu.py compares the device with it) ----
TRAIN = dict(S=4, T=20, delay=3, lr=2e-3, mmt=0.9)


def cldnn_net(seed=3):
    """the net of make_layers at trained-size values: filters U[-0.3, 0.3], the affines and the LSTM as tests/test_nnet.py draws them"""
    from oracle.oracle import make_params
    rng = np.random.RandomState(seed)
    P_, Q_ = 1 + (ST - PD) // PS, 1 + (1 + (ST - PD) // PS - POOL) // POOL
    return [("conv", rng.uniform(-0.3, 0.3, (F, N_BLOCKS * PD)).astype(np.float32), rng.uniform(-0.3, 0.3, F).astype(np.float32), N_BLOCKS * ST, P_ * F, PD, PS, ST),
            ("pool", P_ * F, Q_ * F, POOL, POOL, F), ("sigmoid", Q_ * F),
            ("affine", (0.3 * rng.randn(HID, Q_ * F)).astype(np.float32), (0.1 * rng.randn(HID)).astype(np.float32)),
            ("lstm_streams", make_params(HID, C, R, scale=0.3, seed=seed + 1), HID, C, R, S),
            ("affine", (0.3 * rng.randn(NPDF, R)).astype(np.float32), (0.1 * rng.randn(NPDF)).astype(np.float32)), ("softmax", NPDF)]


def cldnn_utts(seed=5):
    """four utterances, one per stream, of at most T x 5 - delay frames: exactly five minibatches"""
    rng = np.random.RandomState(seed)
    return [(rng.randn(n, N_BLOCKS * ST).astype(np.float32), rng.randint(0, NPDF, n)) for n in (97, 83, 90, 61)]


def cldnn_ctc_utts(seed=9):
    """four utterances of falling length with 3 to 5 labels out of 1 .. NPDF - 1 (0 is the blank): one whole-utterance minibatch"""
    rng = np.random.RandomState(seed)
    return [(rng.randn(n, N_BLOCKS * ST).astype(np.float32), rng.randint(1, NPDF, m)) for n, m in ((30, 5), (26, 4), (22, 4), (17, 3))]


def ctc_diff(y, lens, labels, blank, dt):
    """-log p(labels | y) per stream and its derivative with respect to the Softmax INPUT, from posteriors y [T, S, K] kept in dtype dt
    (tests/ctc_ref.py oracle, which takes float32 posteriors only): torch's ctc_loss on log y; padding rows come back zero"""
    import torch.nn.functional as Fn
    tdt = torch.float64 if dt == np.float64 else torch.float32
    a = torch.log(torch.clamp_min(torch.as_tensor(y, dtype=tdt), float(np.finfo(np.float32).tiny))).requires_grad_()
    flat = torch.tensor([c for lab in labels for c in lab], dtype=torch.long)
    loss = Fn.ctc_loss(Fn.log_softmax(a, -1), flat, torch.tensor(lens), torch.tensor([len(lab) for lab in labels]), blank=blank,
                       reduction="none", zero_infinity=True)
    loss.sum().backward()
    return loss.detach().numpy(), a.grad.numpy().astype(dt)


def cldnn_train(layers, utts, dt, S, T, delay, lr, mmt, ctc_utts=None):
    """bd-nnet-train-lstm-streams.cc's loop (oracle_train of tests/test_nnet.py) over the CLDNN, every piece in dtype dt: cnn_ref for the
    front end, oracle/components.py and the LSTM oracle behind it; components last to first, backpropagate then update, as
    Nnet::Backpropagate does.  With ctc_utts: then one minibatch of TrainCtcWholeUtterances on the same model (momentum buffers kept;
    the utterances zero-padded to the longest, every stream from zero state, the diff rows of the padding zero), and a last forward
    pass over that minibatch.  Returns the stream minibatch count, the parameter tensors by name, and (posteriors [T, S, K], lens) of
    the last pass or None."""
    from oracle import components as oc
    from oracle.oracle import Oracle
    from tests import ctc_ref, kaldi_fmt
    conv, pool, aff1, lstm_l, aff2 = layers[0], layers[1], layers[3], layers[4], layers[5]
    geom, pgeom = conv[5:8], pool[3:6]
    par = dict(Wf=conv[1].astype(dt), bf=conv[2].astype(dt), W1=aff1[1].astype(dt), b1=aff1[2].astype(dt), W2=aff2[1].astype(dt), b2=aff2[2].astype(dt))
    cor = {k_: np.zeros_like(v) for k_, v in par.items()}
    lstm = Oracle(HID, C, R, S, dt)
    lstm.set_params(lstm_l[1])
    flr, fmm = dt(np.float32(lr)), dt(np.float32(mmt))

    def forward(feat, flags):
        x = feat.astype(dt)
        h1 = cnn_ref.conv_forward(x, par["Wf"], par["bf"], geom, dt)
        h2 = cnn_ref.pool_forward(h1, pgeom)
        y = cnn_ref.activation(cnn_ref.SIGMOID, h2, dt)
        a1 = oc.affine_propagate(y, par["W1"], par["b1"])
        lstm.reset(flags)
        r = lstm.propagate(a1)
        return (x, h1, h2, y, a1, r), oc.softmax(oc.affine_propagate(r, par["W2"], par["b2"]))

    def backward(state, diff):
        x, h1, h2, y, a1, r = state
        d_r = oc.affine_backpropagate(diff, par["W2"])
        oc.affine_update(r, diff, par["W2"], par["b2"], cor["W2"], cor["b2"], flr, flr, fmm)
        d_a1 = lstm.backpropagate(a1, d_r, momentum=float(fmm)).astype(dt)
        lstm.update(float(flr))
        d_y = oc.affine_backpropagate(d_a1, par["W1"])
        oc.affine_update(y, d_a1, par["W1"], par["b1"], cor["W1"], cor["b1"], flr, flr, fmm)
        d_h1 = cnn_ref.pool_backward(h1, h2, cnn_ref.activation_diff(cnn_ref.SIGMOID, y, d_y, dt), pgeom)
        fg, bg = cnn_ref.conv_gradient(x, d_h1, geom, F, dt)
        par["Wf"], cor["Wf"] = cnn_ref.sgd_step(par["Wf"], cor["Wf"], fg, lr, mmt, dt)
        par["bf"], cor["bf"] = cnn_ref.sgd_step(par["bf"], cor["bf"], bg, lr, mmt, dt)

    batcher = oc.MultiStreamBatcher(utts, S, T, delay)
    nb = 0
    while True:
        nxt = batcher.next()
        if nxt is None:
            break
        feat, target, mask, flags = nxt
        state, post = forward(feat, flags)
        backward(state, oc.xent_eval_masked(post, target, mask.astype(dt))[0].astype(dt))
        nb += 1
    last = None
    if ctc_utts is not None:
        batches, skipped = ctc_ref.batch_twin(ctc_utts, S, True, 65535 // S)
        assert len(batches) == 1 and skipped == 0
        b = batches[0]
        state, post = forward(b["feat"], [1] * S)
        _, diff = ctc_diff(post.reshape(b["T"], S, NPDF), b["lens"], b["labels"], 0, dt)
        backward(state, diff.reshape(b["T"] * S, NPDF))
        last = (forward(b["feat"], [1] * S)[1].reshape(b["T"], S, NPDF), b["lens"])
    names = ["w_gifo_x", "w_gifo_r", "bias", "peephole_i_c", "peephole_f_c", "peephole_o_c", "w_r_m"]
    out = {"filters": par["Wf"], "conv bias": par["bf"], "affine 1 W": par["W1"], "affine 1 b": par["b1"]}
    out.update({"lstm " + n: a for n, a in zip(names, kaldi_fmt.parts(lstm.get_params(), HID, C, R))})
    out.update({"affine 2 W": par["W2"], "affine 2 b": par["b2"]})
    return nb, out, last


def decided_rows(y64, y32, lens):
    """the rows of the last pass on which the arg-max path is beyond doubt: valid frames whose float64 top-two margin exceeds the
    float32 twin's error on the posteriors (the largest over the valid rows).  Returns (mask [T, S], arg-max of the twin [T, S], error)."""
    T, S, _ = y64.shape
    valid = np.arange(T)[:, None] < np.asarray(lens)[None, :]
    err = float(np.abs(y32.astype(np.float64) - y64)[valid].max())
    top = np.sort(y64, axis=-1)
    return valid & (top[..., -1] - top[..., -2] > err), y32.argmax(-1), err


def test_the_training_reference_runs_five_minibatches_and_its_float32_form_stays_near_float64():
    """what tests/test_cnn_gpu.py holds the device against: five stream minibatches (S = 4, T = 20) and one CTC minibatch, every tensor
    moved, the float32 run within 1e-4 of the float64 run (no max flips its pool, no overflow: the comparison on the device is
    meaningful).  And the seed of the data: the twin alone leaves at most 5 % of the valid rows of the last pass undecided, and agrees
    with the float64 arg-max on every decided row."""
    layers, utts, cu = cldnn_net(), cldnn_utts(), cldnn_ctc_utts()
    nb, p64, (y64, lens) = cldnn_train(layers, utts, np.float64, ctc_utts=cu, **TRAIN)
    nb32, p32, (y32, _) = cldnn_train(layers, utts, np.float32, ctc_utts=cu, **TRAIN)
    nb5, q64, none = cldnn_train(layers, utts, np.float64, **TRAIN)
    assert nb == nb32 == nb5 == 5 and none is None
    for name, a in p64.items():
        e = cnn_ref.rel_err(p32[name], a)
        print(name, a.shape, "float32 run:", e)
        assert np.isfinite(a).all() and e < 1e-4, name
        assert np.abs(a - q64[name]).max() > 1e-6, name + ": the CTC minibatch did not move it"
    for name, a in {"filters": layers[0][1], "affine 1 W": layers[3][1], "affine 2 b": layers[5][2]}.items():
        assert np.abs(q64[name] - a).max() > 1e-4, name + " did not move"
    decided, path, err = decided_rows(y64, y32, lens)
    valid = int(sum(lens))
    print("twin's error on the posteriors", err, "undecided rows", valid - int(decided.sum()), "of", valid)
    assert valid - int(decided.sum()) <= 0.05 * valid
    assert np.array_equal(path[decided], y64.argmax(-1)[decided])
