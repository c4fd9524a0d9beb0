"""Forward-connection dropout on the GPU (kdrop_apply, include/klstm_dropout.h): bit identity to the numpy twin (tests/dropout_ref.py)
on every code path of the kernel, the copy at p == 1, one mask per (stream, sequence), the backward pass, kaldi_lstm_amd.Dropout,
and the <Dropout> component inside TrainLstmStreams / TrainCtcWholeUtterances through tests/cpp/dropout_test.cpp."""
import numpy as np
import pytest
import torch

from oracle import components as oc
from oracle.oracle import Oracle
from tests import dropout_fmt, dropout_ref
from tests.test_component import _pack_utts
from tests.test_dropout import run
from tests.test_nnet import I, C, R, NPDF, make_net

pytestmark = pytest.mark.gpu
f32 = np.float32
SENTINEL = 12345.0
HIGH_SEED = (0xDEADBEEF << 32) | 77
RET, DSEED, DSALT = f32(0.8), 0x0123456789, 2           # the trainer test: the <Dropout> is component 2 of its net, hence its salt
COUNTERS = [(f32(0.5), 1234, 3, 1), (f32(0.8), HIGH_SEED, 2 ** 32 - 1, 5), (f32(2.0 ** -8), 1234, 0, 2 ** 31 - 1),
            (np.nextafter(f32(1), f32(0)), 5, 1, 0)]       # (retention, seed, step, salt)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def block(rows, cols, seed=0):
    """negatives, -0.0, a NaN, both infinities and a denormal among ordinary numbers"""
    x = np.random.RandomState(seed).randn(rows, cols).astype(np.float32)
    flat = x.reshape(-1)
    for i, v in enumerate([-0.0, np.nan, np.inf, -np.inf, 1e-40, 0.0]):
        flat[(i * 7 + 1) % flat.size] = v
    return x


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
    view.copy_(torch.from_numpy(x))
    return view, buf


def padding_intact(view, buf, layout):
    if layout == "contiguous":
        return True
    b = buf.cpu().numpy().copy()
    lo = 1 if layout == "offset" else 0
    b[:, lo:lo + view.shape[1]] = SENTINEL
    return bool((b == SENTINEL).all())


def device_apply(x, layout_in, layout_out, p, seed, step, salt, **kw):
    import kaldi_lstm_amd as k
    vin, _ = placed(x, layout_in)
    vout, bout = placed(np.full_like(x, SENTINEL), layout_out)
    k.dropout_apply(vin, vout, p, seed, step, salt, **kw)
    torch.cuda.synchronize()
    assert padding_intact(vout, bout, layout_out), "columns from cols up to the stride were written"
    return vout.cpu().numpy()


@pytest.mark.parametrize("p,seed,step,salt", COUNTERS)
def test_small_block_is_the_twins_on_every_path(p, seed, step, salt):
    """7 x 37: contiguous (unaligned rows: the scalar path and the tail quad), inside a stride-64 buffer (the vector path plus the
    tail), and the same block one float into a row (a misaligned base): one mask, the twin's, and the padding keeps its sentinel"""
    x = block(7, 37)
    want = bits(dropout_ref.apply(x, p, seed, step, salt))
    for lin, lout in (("contiguous", "contiguous"), ("padded", "padded"), ("offset", "offset"), ("padded", "contiguous"), ("contiguous", "offset")):
        got = bits(device_apply(x, lin, lout, p, seed, step, salt))
        assert np.array_equal(got, want), (lin, lout, int((got != want).sum()))
    keep = dropout_ref.mask(7, 37, p, seed, step, salt)
    assert (want[~keep] == 0).all()                        # +0.0 as such, over the NaN and the infinities too


@pytest.mark.parametrize("p,seed,step,salt", COUNTERS[:2])
def test_in_place(p, seed, step, salt):
    import kaldi_lstm_amd as k
    x = block(5, 64, seed=1)
    v, _ = placed(x, "contiguous")
    k.dropout_apply(v, v, p, seed, step, salt)
    assert np.array_equal(bits(v.cpu().numpy()), bits(dropout_ref.apply(x, p, seed, step, salt)))
    x = block(5, 37, seed=2)                               # and through the scalar path with a tail, in a padded buffer
    v, buf = placed(x, "offset")
    k.dropout_apply(v, v, p, seed, step, salt)
    assert np.array_equal(bits(v.cpu().numpy()), bits(dropout_ref.apply(x, p, seed, step, salt))) and padding_intact(v, buf, "offset")


@pytest.mark.parametrize("rows,cols", [(70000, 5), (3, 16625), (9000, 260)])
def test_large_indices_are_the_twins(rows, cols):
    """70000 x 5: a row index beyond 65535; 3 x 16625: the quad index at the output layer's width; 9000 x 260: 585000 quads, more than
    one pass of the capped grid (2048 x 256 lanes) holds, so the (row, quad) pair is stepped, with a remainder"""
    x = block(rows, cols, seed=3)
    for p, seed, step, salt in COUNTERS[:2]:
        want = bits(dropout_ref.apply(x, p, seed, step, salt))
        for layout in ("contiguous", "padded"):
            assert np.array_equal(bits(device_apply(x, layout, layout, p, seed, step, salt)), want), (p, layout)


def test_retention_one_is_a_copy_bit_for_bit():
    import kaldi_lstm_amd as k
    for rows, cols in ((7, 37), (70000, 5)):
        x = block(rows, cols, seed=4)
        for layout in ("contiguous", "padded", "offset"):
            assert np.array_equal(bits(device_apply(x, layout, layout, 1.0, 1234, 3, 1)), bits(x))
    v, _ = placed(block(5, 64), "contiguous")
    before = bits(v.cpu().numpy())
    k.dropout_apply(v, v, 1.0, 1234, 3, 1)
    assert np.array_equal(bits(v.cpu().numpy()), before)


def test_sequence_mode_one_mask_per_stream_and_sequence():
    S, T, cols, p, seed, salt = 3, 5, 37, f32(0.5), HIGH_SEED, 4
    ids = [7, 7, 9]
    x = block(T * S, cols, seed=5)
    x[np.isnan(x) | np.isinf(x)] = 1.5                     # (so that every kept element shows)
    x[x == 0] = 2.5
    dev_ids = torch.tensor(ids, dtype=torch.int32, device="cuda")
    want = dropout_ref.apply(x, p, seed, 0, salt, dropout_ref.SEQUENCE, S, ids)
    for layout in ("contiguous", "padded", "offset"):
        for step in (0, 17):                               # the step plays no part
            got = device_apply(x, layout, layout, p, seed, step, salt, mode=1, num_stream=S, seq_ids=dev_ids)
            assert np.array_equal(bits(got), bits(want)), layout
    kept = (got != 0).reshape(T, S, cols)
    assert (kept == kept[0]).all()                         # every row of a stream carries that stream's mask
    assert (kept[0, 0] == kept[0, 1]).all()                # streams 0 and 1 share id 7
    assert (kept[0, 2] == dropout_ref.mask(1, cols, p, seed, 0, salt, dropout_ref.SEQUENCE, 1, [9])[0]).all() and not (kept[0, 2] == kept[0, 0]).all()
    elem = device_apply(x, "contiguous", "contiguous", p, seed, 0, salt)
    assert not np.array_equal(elem != 0, got != 0)         # ELEMENT mode with the same seed is another mask
    # many frames of few streams (the rows of a stream are split over lanes) and a row count that is no multiple of S
    for rows, cols2, S2 in ((1500 * 2, 12, 2), (3001, 8, 4), (2, 40, 5)):
        x2 = block(rows, cols2, seed=6)
        ids2 = [2 ** 32 - 1, 0, 3, 3, 8][:S2]
        dev2 = torch.tensor(np.array(ids2, dtype=np.uint32).view(np.int32), device="cuda")
        got2 = device_apply(x2, "padded", "contiguous", p, seed, 0, salt, mode=1, num_stream=S2, seq_ids=dev2)
        assert np.array_equal(bits(got2), bits(dropout_ref.apply(x2, p, seed, 0, salt, dropout_ref.SEQUENCE, S2, ids2))), (rows, cols2, S2)


def test_python_dropout_forward_backward_and_replay():
    import kaldi_lstm_amd as k
    p, seed, salt = f32(0.8), HIGH_SEED, 3
    x, od = block(40, 24, seed=7), np.random.RandomState(8).randn(40, 24).astype(np.float32)
    xd, odd = torch.from_numpy(x).cuda(), torch.from_numpy(od).cuda()
    d = k.Dropout(p, seed=seed, salt=salt)
    assert not d.training
    assert np.array_equal(bits(d.forward(xd).cpu().numpy()), bits(x)) and d.step == 0          # default off: a copy, no step
    assert np.array_equal(bits(d.backward(odd).cpu().numpy()), bits(od))
    d.training = True
    runs = []
    for _ in range(2):
        d.set_seed(seed)
        outs = []
        for step in range(3):
            y = d.forward(xd).cpu().numpy()
            g = d.backward(odd).cpu().numpy()
            assert d.step == step + 1
            keep = dropout_ref.mask(40, 24, p, seed, step, salt)
            _, scale = dropout_ref.threshold(p)
            assert np.array_equal(bits(y), bits(dropout_ref.apply(x, p, seed, step, salt)))
            assert np.array_equal(bits(g), bits(np.where(keep, od * scale, f32(0))))           # in_diff = out_diff . mask . scale
            outs += [y, g]
        runs.append(outs)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(*runs))                        # two runs: bit-identical
    # per sequence: ids from the layer's counter at every flagged reset
    d = k.Dropout(p, seed=seed, salt=salt, per_sequence=True)
    d.training = True
    S = 4
    xs = block(5 * S, 24, seed=9)
    xsd = torch.from_numpy(xs).cuda()
    d.reset([1, 1, 1, 1])                                                                      # ids 0 1 2 3
    y0 = d.forward(xsd).cpu().numpy()
    assert np.array_equal(bits(y0), bits(dropout_ref.apply(xs, p, seed, 0, salt, dropout_ref.SEQUENCE, S, [0, 1, 2, 3])))
    d.reset([0, 1, 0, 0])                                                                      # stream 1 starts sequence 4; the others carry on
    y1 = d.forward(xsd).cpu().numpy()
    assert np.array_equal(bits(y1), bits(dropout_ref.apply(xs, p, seed, 0, salt, dropout_ref.SEQUENCE, S, [0, 4, 2, 3])))
    assert np.array_equal(bits(d.backward(xsd).cpu().numpy()), bits(y1))
    with pytest.raises(k.KlstmError):
        k.Dropout(0.0)


# ---- the <Dropout> component (tests/cpp/dropout_test.cpp) ----
@pytest.mark.parametrize("per_sequence", [0, 1])
def test_cpp_layer_counts_steps_and_sequences_like_the_twin(tmp_path, per_sequence):
    """Transmit -> Dropout 0.8 through Nnet::Propagate / Backpropagate: off it is a copy; on, minibatch k carries the twin's mask of
    step k and salt 1 (the component's index), or of the sequence ids the Resets handed out; the backward pass replays it"""
    S, T, cols, seed = 4, 6, 20, HIGH_SEED
    x = np.random.RandomState(10).randn(T * S, cols).astype(np.float32)
    x.tofile(tmp_path / "x.raw")
    assert run("layer", tmp_path / "x.raw", T * S, cols, seed, per_sequence, tmp_path / "y.raw").stdout.split() == ["OK", "3"]
    got = np.fromfile(tmp_path / "y.raw", dtype=np.float32).reshape(4, 2, T * S, cols)
    assert np.array_equal(bits(got[0, 0]), bits(x)) and np.array_equal(bits(got[0, 1]), bits(x))       # default off
    ids = [[0, 1, 2, 3], [0, 4, 2, 3], [0, 4, 2, 3]]
    for k in range(3):
        if per_sequence:
            want = dropout_ref.apply(x, RET, seed, 0, 1, dropout_ref.SEQUENCE, S, ids[k])
        else:
            want = dropout_ref.apply(x, RET, seed, k, 1)
        assert np.array_equal(bits(got[k + 1, 0]), bits(want)) and np.array_equal(bits(got[k + 1, 1]), bits(want)), k


# ---- the <Dropout> component in the trainers ----


def oracle_train_dropout(flat, W, b, utts, S, T, delay, lr, mmt, crossvalidate=False):
    """oracle_train of tests/test_nnet.py (bd-nnet-train-lstm-streams.cc:143-304 with the oracle pieces) with the twin's masks between
    the LSTM and the Affine, forward and backward; step = the minibatch, as the layer counts it.  Cross-validation leaves them out."""
    lstm = Oracle(I, C, R, S, np.float32); lstm.set_params(flat)
    W, b = W.copy(), b.copy(); Wc, bc = np.zeros_like(W), np.zeros_like(b)
    batcher = oc.MultiStreamBatcher(utts, S, T, delay)
    loss = correct = frames = 0.0
    nb = 0
    while True:
        nxt = batcher.next()
        if nxt is None:
            break
        feat, target, mask, flags = nxt
        lstm.reset(flags)
        h = lstm.propagate(oc.transmit(feat))
        hd = h if crossvalidate else dropout_ref.apply(h, RET, DSEED, nb, DSALT)
        a = oc.affine_propagate(hd, W, b); y = oc.softmax(a)
        diff, xe, ent, cor, valid = oc.xent_eval_masked(y, target, mask)
        loss += xe - ent; correct += cor; frames += valid
        if not crossvalidate:
            d_hd = oc.affine_backpropagate(diff, W)
            oc.affine_update(hd, diff, W, b, Wc, bc, lr, lr, mmt)
            d_h = dropout_ref.apply(d_hd, RET, DSEED, nb, DSALT)
            lstm.backpropagate(feat, d_h, momentum=mmt); lstm.update(lr)
        nb += 1
    return dict(loss=loss / frames, acc=correct / frames, frames=frames, nb=nb, lstm=lstm.get_params(), W=W, b=b)


def numbers(path):
    return np.array([float(v) for v in path.read_text().replace("[", " ").replace("]", " ").split() if v[0] in "-0123456789."])


@pytest.mark.parametrize("crossvalidate", [0, 1])
def test_train_lstm_streams_with_dropout_end_to_end(tmp_path, crossvalidate):
    """Transmit -> LSTM(8 -> 16 -> 8) -> Dropout 0.8 -> Affine -> Softmax, S = 4, T = 10: the shapes and data of
    tests/test_nnet.py::test_train_lstm_streams_workalike_end_to_end and its bars (2e-4 on the loss, 1.5 / frames on the accuracy, 1e-3
    of the largest parameter): the feature adds exact selections and one correctly rounded multiply."""
    S, T, delay, lr, mmt = 4, 10, 3, 2e-3, 0.9
    layers, flat, W, b = make_net(S, seed=3)
    layers = layers[:2] + [("dropout", R, float(RET))] + layers[2:]
    rng = np.random.RandomState(5)
    utts = [(rng.randn(n, I).astype(np.float32), rng.randint(0, NPDF, n)) for n in (37, 10, 52, 25, 8, 61, 30)]
    (tmp_path / "n.bin").write_bytes(dropout_fmt.nnet_binary(layers))
    _pack_utts(utts).tofile(tmp_path / "u.raw")
    r = run("train", tmp_path / "n.bin", tmp_path / "u.raw", S, T, delay, lr, mmt, crossvalidate, 0, DSEED, tmp_path / "out.bin")
    lines = r.stdout.splitlines()
    head = lines[0].split()
    exp = oracle_train_dropout(flat, W, b, utts, S, T, delay, lr, mmt, bool(crossvalidate))
    print("loss", head[4], exp["loss"], "acc", head[5], exp["acc"])
    assert head[0] == "OK" and int(head[1]) == len(utts) and int(head[2]) == exp["nb"] and float(head[3]) == exp["frames"]
    assert head[6] == "restored" and head[7] == "1"                                   # the active state is put back
    assert abs(float(head[4]) - exp["loss"]) <= 2e-4 * abs(exp["loss"])
    assert abs(float(head[5]) - exp["acc"]) <= 1.5 / exp["frames"]
    if crossvalidate:
        cv = lines[1].split()
        assert cv[0] == "CV" and cv[1] == cv[2] and cv[3] == cv[4]                    # the loss of the WithoutDropout form, bit for bit
        assert not (tmp_path / "out.bin").exists()
    else:
        trained = [("transmit", I), ("lstm_streams", exp["lstm"], I, C, R, S), ("dropout", R, float(RET)), ("affine", exp["W"], exp["b"]), ("softmax", NPDF)]
        (tmp_path / "exp.bin").write_bytes(dropout_fmt.nnet_binary(trained))
        run("nnet_copy", tmp_path / "out.bin", 0, tmp_path / "out.txt")
        run("nnet_copy", tmp_path / "exp.bin", 0, tmp_path / "exp.txt")
        got, want = numbers(tmp_path / "out.txt"), numbers(tmp_path / "exp.txt")
        print("largest parameter difference", np.abs(got - want).max(), "of", np.abs(want).max())
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-3 * np.abs(want).max()


def test_ctc_trainer_per_sequence_replays_and_decodes_like_the_model_without_dropout():
    """tests/cpp/dropout_test.cpp ctc: a two-layer stack with a <Dropout> between the layers at S = 3; two runs with one seed give
    bit-identical models, a second seed (and the per-element mode) another one; DecodeCtcWholeUtterances gives the hypotheses of the
    WithoutDropout form"""
    out = run("ctc").stdout
    assert out.startswith("OK models ") and " 12 hypotheses" in out
