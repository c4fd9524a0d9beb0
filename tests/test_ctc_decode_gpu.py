"""klstm_ctc_decode on the device (kaldi_lstm_amd.ctc_greedy_decode) against its numpy twin (tests/ctc_decode_ref.py).

Every integer the call produces -- frame_class, hyp, hyp_len, errors, the five totals -- must EQUAL the twin: there is no tolerance to
choose.  The one float, `score`, is measured against the float64 sum of log(max(y_best, FLT_MIN)) over the twin's path; its bar is what
stock float32 delivers on the same input (numpy log in float32, summed sequentially in float32; never the kernel): the kernel sums
float32 logs in double and rounds once, so no extra margin is given.  Weighted cases keep y in {0} U [2^-100, 1] and w in
[2^-20, 2^20]: no product is subnormal and the float32 twin is exact whatever the denormal mode of the kernel."""
import numpy as np
import pytest
import torch

import kaldi_lstm_amd as k
from tests import ctc_decode_ref as D
from tests import ctc_ref as R
from tests.margins import bound

pytestmark = pytest.mark.gpu

LENS_A = [300, 299, 250, 180, 120, 61, 30, 7]
LABS_A = [40, 60, 33, 50, 60, 30, 29, 3]


def gpu_decode(y, lens, blank, w=None, refs=None, off=0, totals=None):
    """y [T, S, K] float32 numpy.  off > 0: net_out is a column window that starts `off` columns into a wider matrix of odd width."""
    y = np.ascontiguousarray(y, dtype=np.float32)
    T, S, K = y.shape
    flat = torch.from_numpy(y.reshape(T * S, K))
    if off:
        width = K + off + 2 + (K + off) % 2                       # odd: every other row starts off a 16-byte boundary differently
        yw = torch.full((T * S, width), 7.0, device="cuda")
        yw[:, off:off + K] = flat.cuda()
        yd = yw[:, off:off + K]
        assert yd.data_ptr() % 16 != 0 or yd.stride(0) % 4 != 0
    else:
        yd = flat.cuda().contiguous()
    y0 = yd.clone()
    wd = None if w is None else torch.from_numpy(np.asarray(w, np.float32)).cuda()
    res = k.ctc_greedy_decode(yd, lens, blank=blank, class_weight=wd, refs=refs, totals=totals)
    torch.cuda.synchronize()
    assert yd.cpu().numpy().tobytes() == y0.cpu().numpy().tobytes(), "the posterior matrix was modified"
    if off:
        assert bool((yw[:, :off] == 7.0).all()) and bool((yw[:, off + K:] == 7.0).all()), "columns outside the window were touched"
    return res


def check(y, lens, blank, w=None, refs=None, off=0):
    """everything the call returns against the twin, exactly; -> (result, twin)"""
    T, S, K = y.shape
    tw = D.decode_twin(y, lens, blank, w, refs)
    totals = torch.zeros(5, dtype=torch.float64, device="cuda") if refs is not None else None
    res = gpu_decode(y, lens, blank, w, refs, off, totals)
    fc = res.frame_class.cpu().numpy().reshape(T, S)
    bad = np.argwhere(fc != tw["frame_class"])
    assert bad.size == 0, f"frame_class differs at (t, s) = {bad[:5].tolist()}: gpu {fc[tuple(bad[0])]} twin {tw['frame_class'][tuple(bad[0])]}"
    assert res.hyp.shape == (S, T) and res.hyp.dtype == torch.int32
    assert k.hypotheses_to_lists(res.hyp, res.hyp_len) == tw["hyp"]
    if refs is None:
        assert res.errors is None
    else:
        assert res.errors.cpu().tolist() == tw["errors"]
        assert totals.cpu().tolist() == tw["totals"]
    return res, tw


def random_refs(seed, K, blank, lab_lens):
    rng = np.random.RandomState(seed)
    out = []
    for n in lab_lens:
        lab = rng.randint(0, K - 1, n)
        out.append((lab + (lab >= blank)).tolist())
    return out


def weights(seed, K):
    return (2.0 ** np.random.RandomState(seed).uniform(-20, 20, K)).astype(np.float32)


def clean(y):
    """into {0} U [2^-100, 1] for the weighted cases"""
    y = np.asarray(y, np.float32).copy()
    y[y < np.float32(2.0 ** -100)] = 0
    return y


# ---------------------------------------------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------------------------------------------
def test_ragged_random_posteriors():
    y, _ = R.make_case(1, 300, 48, 3.0, LENS_A, LABS_A)
    y = clean(y.numpy())
    refs = random_refs(1, 48, 0, LABS_A)
    res, tw = check(y, LENS_A, 0, refs=refs)
    assert len(tw["hyp"][0]) > 200 and tw["errors"][0] > 200          # random posteriors: about one error per reference token and more
    check(y, LENS_A, 0, w=weights(2, 48), refs=refs)


@pytest.mark.parametrize("K", [2, 29, 63, 64, 65, 4097, 16624, 32768])
def test_class_counts_blank_positions_weights(K):
    T = 40 if K <= 4097 else 12
    lens = [T, T - 3, 0, T // 2, 1]
    y, _ = R.make_case(K, T, K, 4.0, lens, [0] * 5)
    y = clean(y.numpy())
    for blank in sorted({0, K - 1, K // 2}):
        refs = random_refs(K + blank, K, blank, [7, 0, 3, 12, 2]) if K > 2 else [[1 - blank] * n for n in (7, 0, 3, 12, 2)]
        check(y, lens, blank, refs=refs)
        check(y, lens, blank, w=weights(K, K), refs=refs)


@pytest.mark.parametrize("S,T,K", [(1, 65535, 4), (4, 500, 48), (8, 300, 130), (32, 100, 48), (15, 4369, 5), (32, 2047, 3), (4, 1100, 2100)])
def test_stream_counts_and_row_limit(S, T, K):
    lens = [T - (53 * s) % (T // 2) for s in range(S)]
    lens[0] = T
    y, _ = R.make_case(S + T, T, K, 1.0, lens, [0] * S)
    refs = random_refs(S, K, 0, [min(20 + s, 40) for s in range(S)])
    check(y.numpy(), lens, 0, refs=refs)


@pytest.mark.parametrize("K,off", [(48, 1), (65, 3), (300, 5), (4097, 7)])
def test_column_window_with_odd_offset(K, off):
    lens = [30, 29, 17, 0, 5]
    y, _ = R.make_case(K + off, 30, K, 3.0, lens, [0] * 5)
    y = clean(y.numpy())
    refs = random_refs(off, K, K // 2, [5, 6, 7, 8, 0])
    check(y, lens, K // 2, refs=refs, off=off)
    check(y, lens, K // 2, w=weights(off, K), refs=refs, off=off)


# ---------------------------------------------------------------------------------------------------------------------------------
# ties, NaN, inf, zeros; what padding holds does not matter
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,min_rows", [(16, 0), (63, 0), (65, 0), (128, 0), (256, 0), (257, 0), (300, 0), (1030, 0), (2048, 0), (4097, 0),
                                        (9000, 0), (4100, 4200)])     # the last: enough rows for the wave-per-row kernel at K > 2048
@pytest.mark.parametrize("off", [0, 3])
def test_planted_ties_nan_inf(K, min_rows, off):
    """equal maxima in several columns: neighbours inside one 16-byte load, either side of a load, of a lane's stride (4 x 16, 4 x 64,
    4 x 256 columns apart), of the scalar head and tail, first and last column; NaN and +inf inside valid rows; rows of zeros, of NaN"""
    rng = np.random.RandomState(K)
    pairs = [(0, K - 1), (1, 2), (3, 4), (K - 2, K - 1), (K // 2, K // 2 + 1)]
    for d in (4, 64, 256, 1024, 63, 255, 257):
        for a in (0, 1, 2, 3, 5):
            if a + d < K:
                pairs.append((a, a + d))
                pairs.append((K - 1 - a - d, K - 1 - a))
    rows = max(2 * len(pairs) + 40, min_rows)
    T, S = (rows + 2) // 3 + 1, 3
    lens = [T, T, T - 1]
    y = (rng.rand(T, S, K).astype(np.float32) * np.float32(0.5) + np.float32(2.0 ** -20))
    flat = y.reshape(T * S, K)
    for i, (a, b) in enumerate(pairs):
        flat[2 * i, [a, b]] = 0.75                                      # two equal maxima
        flat[2 * i + 1, [a, b]] = 0.75
        flat[2 * i + 1, rng.randint(0, K)] = np.nan                     # ... and a NaN somewhere (perhaps on one of them)
    base = 2 * len(pairs)
    flat[base] = 0.0
    flat[base + 1] = np.nan
    flat[base + 2, :] = 0.25                                            # all equal
    flat[base + 3, K - 1] = np.inf
    flat[base + 4, [K // 3, K - 1]] = np.inf
    flat[base + 5, :] = np.nan
    flat[base + 5, K - 1] = 0.0                                         # a single number among NaN
    for r in range(base + 6, base + 40):                                # three to five equal maxima at random places
        flat[r, rng.choice(K, size=min(K, rng.randint(3, 6)), replace=False)] = 0.875
    res, tw = check(y, lens, 0, off=off)
    fc = tw["frame_class"].reshape(-1)
    assert fc[base] == 0 and fc[base + 1] == 0 and fc[base + 2] == 0 and fc[base + 3] == K - 1 and fc[base + 4] == K // 3 and fc[base + 5] == K - 1


@pytest.mark.parametrize("K", [48, 300, 4097])
def test_equal_products_from_different_factors(K):
    rng = np.random.RandomState(K)
    T, S = 50, 2
    y = rng.rand(T, S, K).astype(np.float32) * np.float32(2.0 ** -16) + np.float32(2.0 ** -30)       # times w <= 8: below 2^-11
    w = np.ones(K, np.float32)
    cols = rng.choice(K, size=6, replace=False)
    w[cols] = [2.0, 4.0, 0.5, 8.0, 1.0, 2.0 ** -10]
    for t in range(T):
        for s in range(S):
            pick = rng.choice(cols, size=rng.randint(2, 5), replace=False)
            y[t, s, pick] = np.float32(2.0 ** -11) / w[pick]            # exact: powers of two.  Products 2^-11 in every picked column
    res, tw = check(y, [T, T - 7], 0, w=w)
    assert set(np.unique(tw["frame_class"][:T - 7])) <= set(cols.tolist())
    check(y, [T, T - 7], 0)                                             # without the weights: the largest y, another column


def test_padding_and_idle_streams_are_not_read():
    lens = [60, 0, 41, 7, 60, 61]                                       # stream 5: longer than T, rejected
    T, S, K = 60, 6, 300
    y0, _ = R.make_case(3, T, K, 3.0, lens, [0] * S)
    y0 = clean(y0.numpy())
    refs = random_refs(3, K, 0, [10, 4, 9, 2, 0, 5])
    w = weights(3, K)
    outs = []
    for fill in (0.0, np.nan, np.inf, 1e38):
        y = y0.copy()
        for s, n in enumerate(lens):
            y[(n if n <= T else 0):, s] = fill
        res, tw = check(y, lens, 0, w=w, refs=refs)
        assert tw["errors"][1] == -1 and tw["errors"][5] == -1 and tw["totals"][3] == 4
        outs.append([res.frame_class.cpu().numpy().tobytes(), res.hyp_len.cpu().numpy().tobytes(), res.score.cpu().numpy().tobytes(),
                     res.errors.cpu().numpy().tobytes(), str(k.hypotheses_to_lists(res.hyp, res.hyp_len))])
        assert res.score.cpu().numpy()[[1, 5]].tolist() == [0.0, 0.0] and res.hyp_len.cpu().tolist()[1] == 0
    assert all(o == outs[0] for o in outs[1:])


# ---------------------------------------------------------------------------------------------------------------------------------
# hypotheses close to their references; the corners of the edit distance
# ---------------------------------------------------------------------------------------------------------------------------------
def test_close_hypotheses():
    K, T = 48, 300
    refs = random_refs(7, K, 0, [40, 60, 33, 50, 60, 30, 29, 3, 80, 70, 64, 63])
    refs[5] = [9] * 30                                                   # one class repeated: a blank between every pair
    lens = [300, 299, 250, 180, 220, 61, 130, 7, 300, 300, 280, 270]
    corrupt = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (0, 0, 0, 0), (2, 2, 2, 2), (0, 0, 0, 0),
               (5, 0, 3, 4), (0, 7, 0, 0), (0, 0, 9, 0), (3, 3, 3, 3)]
    y = D.peaked_case(11, T, K, 0, refs, lens, corrupt)
    res, tw = check(y, lens, 0, refs=refs)
    print("close hypotheses: distances", tw["errors"], flush=True)
    assert tw["errors"][0] == 0 and tw["errors"][5] == 0 and tw["errors"][7] == 0
    assert 0 < min(e for e in tw["errors"] if e > 0) <= 1 and max(tw["errors"]) <= 16
    check(y, lens, 0, w=weights(7, K), refs=refs)


def test_edit_distance_corners():
    """L = 0, H = 0 (all blank), L = 1023, H = T = 2000, reference longer than the hypothesis and the reverse, L either side of the row
    geometries (63 / 64, 255 / 256 reference tokens)"""
    K, T, S = 11, 2000, 12
    rng = np.random.RandomState(5)
    lens = [2000, 2000, 2000, 1500, 2000, 700, 2000, 2000, 300, 300, 900, 900]
    y = rng.rand(T, S, K).astype(np.float32) * np.float32(0.01)
    path = np.zeros((T, S), np.int64)
    path[:, 0] = 1 + (np.arange(T) % 2)                                  # H = T = 2000
    path[:, 1] = 0                                                       # H = 0
    path[:, 2] = 1 + (np.arange(T) % 10)
    for s in range(3, S):
        path[:, s] = np.repeat(rng.randint(0, K, T // 2 + 1), 2)[:T]
    y[np.arange(T)[:, None], np.arange(S)[None, :], path] = 0.9
    near = [c for c, p in zip(path[:lens[6], 6].tolist(), [-1] + path[:lens[6] - 1, 6].tolist()) if c != 0 and c != p]
    refs = [random_refs(1, K, 0, [1023])[0], random_refs(2, K, 0, [5])[0], [], random_refs(3, K, 0, [1023])[0], random_refs(4, K, 0, [1])[0],
            [], near[:1023], random_refs(6, K, 0, [63])[0], random_refs(7, K, 0, [64])[0], random_refs(8, K, 0, [255])[0],
            random_refs(9, K, 0, [256])[0], random_refs(10, K, 0, [700])[0]]
    res, tw = check(y, lens, 0, refs=refs)
    print("edit distance corners: hyp lengths", [len(h) for h in tw["hyp"]], "distances", tw["errors"], flush=True)
    assert len(tw["hyp"][0]) == 2000 and tw["hyp"][1] == [] and tw["errors"][1] == 5 and tw["errors"][2] == 2000
    assert tw["errors"][6] <= max(0, len(near) - 1023)


def test_statuses():
    K, T = 32, 200
    lens = [200, 0, 201, -1, 200, 200, 200, 150]
    y, _ = R.make_case(9, T, K, 2.0, [200] * 8, [0] * 8)
    y = y.numpy()
    refs = random_refs(9, K, 3, [20, 20, 20, 20, 20, 20, 0, 20])
    refs[4][4] = K                                                      # outside [0, K)
    refs[5][0] = 3                                                      # the blank itself
    res, tw = check(y, lens, 3, refs=refs)
    err, n, sc = res.errors.cpu().tolist(), res.hyp_len.cpu().tolist(), res.score.cpu().numpy()
    assert [e >= 0 for e in err] == [True, False, False, False, False, False, True, True]
    assert n[1] == n[2] == n[3] == 0 and sc[1] == sc[2] == sc[3] == 0.0
    assert n[4] > 0 and n[5] > 0 and sc[4] < 0 and sc[5] < 0             # a bad reference: hypothesis and score as usual
    assert err[6] == n[6]                                               # an empty reference
    assert tw["totals"][3] == 3
    fc = res.frame_class.cpu().numpy().reshape(T, 8)
    assert (fc[:, 1:4] == -1).all() and (fc[150:, 7] == -1).all() and (fc[:, 0] >= 0).all()
    # a reference of more than 1023 labels is not counted either
    long_refs = [random_refs(1, K, 3, [1024])[0]] + refs[1:]
    res, tw = check(y, lens, 3, refs=long_refs)
    assert res.errors.cpu().tolist()[0] == -1 and res.hyp_len.cpu().tolist()[0] == n[0] and tw["totals"][3] == 2


def test_bit_identical_runs_and_stream_permutation():
    lens = LENS_A[:5] + [58, 30, 61]
    y, _ = R.make_case(11, 300, 48, 3.0, lens, LABS_A)
    y = y.numpy()
    refs = random_refs(11, 48, 0, LABS_A)

    def run(y, lens, refs):
        r = gpu_decode(y, lens, 0, refs=refs)
        return (k.hypotheses_to_lists(r.hyp, r.hyp_len), r.score.cpu().numpy(), r.errors.cpu().numpy(),
                r.frame_class.cpu().numpy().reshape(y.shape[0], y.shape[1]))
    h1, s1, e1, f1 = run(y, lens, refs)
    h2, s2, e2, f2 = run(y, lens, refs)
    assert h1 == h2 and s1.tobytes() == s2.tobytes() and e1.tobytes() == e2.tobytes() and f1.tobytes() == f2.tobytes()
    perm = [3, 7, 0, 5, 1, 6, 2, 4]
    hp, sp, ep, fp = run(np.ascontiguousarray(y[:, perm]), [lens[p] for p in perm], [refs[p] for p in perm])
    assert hp == [h1[p] for p in perm] and sp.tobytes() == s1[perm].tobytes() and ep.tobytes() == e1[perm].tobytes()
    assert np.ascontiguousarray(fp).tobytes() == np.ascontiguousarray(f1[:, perm]).tobytes()
    h3, s3, e3, f3 = run(np.ascontiguousarray(y[:, :3]), lens[:3], refs[:3])          # fewer neighbours
    assert h3 == h1[:3] and s3.tobytes() == s1[:3].tobytes() and e3.tobytes() == e1[:3].tobytes()


# ---------------------------------------------------------------------------------------------------------------------------------
# the path score
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,T,K,scale", [(1, 300, 48, 3.0), (2, 120, 4097, 8.0), (3, 2000, 29, 1.0)])
def test_score_against_float64(seed, T, K, scale):
    """utterance-length streams only: at a handful of frames float32 summation is nearly exact and the yardstick says nothing"""
    lens = [T, T - 1, (3 * T) // 4, T // 2]
    y, _ = R.make_case(seed, T, K, scale, lens, [0] * 4)
    y = y.numpy()
    res, tw = check(y, lens, 0)
    want = D.path_logp64(y, lens, tw["frame_class"])
    stock = D.path_logp32_stock(y, lens, tw["frame_class"]).astype(np.float64)
    got = res.score.cpu().numpy().astype(np.float64)
    e_gpu = float(np.max(np.abs(got - want) / np.abs(want)))
    e_32 = float(np.max(np.abs(stock - want) / np.abs(want)))
    print(f"ctc decode score T={T} K={K}: gpu {e_gpu:.3g} stock-fp32 {e_32:.3g}", flush=True)
    bound(e_gpu, e_32, "score rel vs fp64 (bar: stock fp32 log + sequential sum)")


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_limits_are_refused():
    lib = k.load_library()
    y = torch.full((4, 8), 0.125, device="cuda")
    for blank in (8, -1):
        with pytest.raises(k.KlstmError) as ei:
            k.ctc_greedy_decode(y, [1, 1, 1, 1], blank=blank)
        assert ei.value.status == 1
    ws = torch.empty(k.ctc_decode_workspace_bytes(1, 4, 1), dtype=torch.uint8, device="cuda")
    lens = torch.ones(4, dtype=torch.int32, device="cuda")
    hyp = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    hlen = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    fc = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((4,), -7.0, device="cuda")

    def call(K, stride, blank, nbytes):
        return lib.klstm_ctc_decode(y.data_ptr(), 1, 4, K, stride, lens.data_ptr(), blank, None, hyp.data_ptr(), hlen.data_ptr(), sc.data_ptr(),
                                    fc.data_ptr(), None, None, None, None, ws.data_ptr(), nbytes, None)
    assert call(1, 8, 0, ws.numel()) == 2 and b"K" in lib.klstm_last_error()
    assert call(32769, 32769, 0, ws.numel()) == 2 and b"32768" in lib.klstm_last_error()
    assert call(8, 8, 8, ws.numel()) == 1 and call(8, 8, -1, ws.numel()) == 1
    assert call(8, 8, 0, ws.numel() - 1) == 1 and b"workspace" in lib.klstm_last_error()
    assert call(8, 4, 0, ws.numel()) == 1                                # a row stride below K
    torch.cuda.synchronize()
    for t in (hyp, hlen, fc):
        assert bool((t == -7).all()), "a refused call wrote an output"
    assert bool((sc == -7.0).all())
    assert call(8, 8, 0, ws.numel()) == 0                                # ... and the same call within the limits runs
    torch.cuda.synchronize()
    assert fc.cpu().tolist() == [0, 0, 0, 0] and hlen.cpu().tolist() == [0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end through the C++ classes (include/klstm_nnet.hpp CtcGreedyDecoder, DecodeCtcWholeUtterances; tests/cpp/ctc_decode_test)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["blstm", "lstm"])
def test_cpp_train_then_decode(tmp_path, kind):
    """The memorisable pattern task, trained with TrainCtcWholeUtterances, the training utterances decoded before and after.
    Bars: token error rate after < before, and after < 1.0 -- a decoder that emits nothing (all blank, where CTC training sits at
    first) scores exactly 1.0, every reference token a deletion, so anything below it means tokens are being recognised.
    Measured: 0.797 -> 0 (bidirectional, 60 epochs), 0.747 -> 0 (unidirectional, 150 epochs; still 1.0 after 60)."""
    from tests.test_ctc_decode import run_driver
    dump = str(tmp_path / "dump.bin")
    r = run_driver("train", kind, dump)
    kv = dict(f.split("=") for f in r.stdout.split() if "=" in f)
    print(f"ctc_decode_test train {kind}:", r.stdout.strip(), flush=True)
    before, after, cv = float(kv["ter_before"]), float(kv["ter_after"]), float(kv["ter_crossvalidate"])
    assert after < before, (before, after)
    assert after < 1.0, after
    assert int(kv["skipped"]) == 1 and int(kv["scored"]) == 12 and int(kv["in_order"]) == 1
    # the every_batch recipe of INTEGRATION.md 3e on a cross-validation pass: the same model, the same utterances, the same rate
    assert cv == after and int(kv["cv_scored"]) == 12
    assert after == int(kv["errors_after"]) / int(kv["ref_tokens"]) or abs(after - int(kv["errors_after"]) / int(kv["ref_tokens"])) < 1e-5
    # the minibatch the driver dumped: Python's ctc_greedy_decode on the same posteriors gives the same bits
    raw = np.fromfile(dump, dtype=np.int32)
    T, S, K, nlab = (int(v) for v in raw[:4])
    p = 4
    lens = raw[p:p + S].tolist(); p += S
    off = raw[p:p + S + 1].tolist(); p += S + 1
    flat = raw[p:p + nlab].tolist(); p += nlab
    post = raw[p:p + T * S * K].view(np.float32).reshape(T * S, K); p += T * S * K
    hlen = raw[p:p + S].tolist(); p += S
    hyp = raw[p:p + S * T].reshape(S, T); p += S * T
    err = raw[p:p + S].tolist(); p += S
    score = raw[p:p + S].view(np.float32); p += S
    fc = raw[p:p + T * S]; p += T * S
    assert p == raw.size
    refs = [flat[off[s]:off[s + 1]] for s in range(S)]
    res = k.ctc_greedy_decode(torch.from_numpy(post.copy()).cuda(), lens, blank=0, refs=refs)
    assert k.hypotheses_to_lists(res.hyp, res.hyp_len) == [hyp[s, :hlen[s]].tolist() for s in range(S)]
    assert res.errors.cpu().tolist() == err and res.score.cpu().numpy().tobytes() == score.tobytes()
    assert res.frame_class.cpu().numpy().tobytes() == fc.tobytes()
    tw = D.decode_twin(post.reshape(T, S, K), lens, 0, refs=refs)
    assert tw["errors"] == err and np.isfinite(score).all()
