"""klstm_ctc_align on the device (kaldi_lstm_amd.ctc_align) against its numpy twin (tests/ctc_align_ref.py).

Two kinds of assertion, because a sum of float32 logs cannot be made bit-reproducible across implementations and a best path has no
tolerance:
  EXACT        on inputs whose best path does not depend on the precision of the chain (peaked posteriors: leaving the best path costs
               of the order of log K nats; uniform posteriors: exact ties, decided by the tie rule; tests/test_ctc_align.py checks on
               the CPU that the float32 and the float64 chain agree on every one of them) every integer output equals the float64 twin.
  OPTIMALITY   on arbitrary posteriors the returned path must be a valid alignment and its float64 score, computed HERE from net_out and
               the returned frame_class, may fall short of the float64 optimum by at most
                   bar = max(sqrt(len) * ulp32(|best64|), 2 * the largest shortfall of the STOCK fp32 chain over the seeds of the shape)
               (the stock chain: tests/ctc_align_ref.align_twin(dtype=float32), run here on the CPU; never the kernel).  A path can
               displace the optimum only if the two computed scores cross, so the shortfall is bounded by the rounding accumulated
               in two path scores: len roundings of at most half an ulp of a partial sum <= |best64|, statistically sqrt(len) * ulp;
               the factor 2 because the kernel's logf and order of operations are another draw from the same distribution.
The float `score` is measured against the float64 sum along the RETURNED path; its bar is the error of stock float32 (numpy log in
float32, summed sequentially in float32) on the same path, no extra margin."""
import numpy as np
import pytest
import torch

import kaldi_lstm_amd as k
from tests import ctc_align_ref as A
from tests import ctc_decode_ref as D
from tests import ctc_ref as R
from tests.margins import bound

pytestmark = pytest.mark.gpu

LENS_A = [300, 299, 250, 180, 120, 61, 30, 7]
LABS_A = [40, 60, 33, 50, 60, 30, 29, 3]


def gpu_align(y, lens, labels, blank, w=None, off=0, totals=None):
    """y [T, S, K] float32 numpy.  off > 0: net_out is a column window that starts `off` columns into a wider matrix of odd width.
    -> dict of numpy arrays: frame_class, frame_pos [T, S]; token_begin, token_end (flat, parallel to the packed labels), offsets,
    score [S]"""
    y = np.ascontiguousarray(y, dtype=np.float32)
    T, S, K = y.shape
    flat = torch.from_numpy(y.reshape(T * S, K))
    if off:
        width = K + off + 2 + (K + off) % 2
        yw = torch.full((T * S, width), 7.0, device="cuda")
        yw[:, off:off + K] = flat.cuda()
        yd = yw[:, off:off + K]
        assert yd.data_ptr() % 16 != 0 or yd.stride(0) % 4 != 0
    else:
        yd = flat.cuda().contiguous()
    y0 = yd.clone()
    wd = None if w is None else torch.from_numpy(np.asarray(w, np.float32)).cuda()
    packed = k.ctc.pack_labels(labels, yd.device)
    res = k.ctc_align(yd, lens, packed, blank=blank, class_weight=wd, totals=totals)
    torch.cuda.synchronize()
    assert yd.cpu().numpy().tobytes() == y0.cpu().numpy().tobytes(), "the posterior matrix was modified"
    if off:
        assert bool((yw[:, :off] == 7.0).all()) and bool((yw[:, off + K:] == 7.0).all()), "columns outside the window were touched"
    nlab = int(packed[1][-1])
    return dict(frame_class=res.frame_class.cpu().numpy().reshape(T, S), frame_pos=res.frame_pos.cpu().numpy().reshape(T, S),
                token_begin=res.token_begin.cpu().numpy()[:nlab], token_end=res.token_end.cpu().numpy()[:nlab],
                offsets=packed[1].cpu().numpy(), score=res.score.cpu().numpy(), result=res)


def check_exact(y, lens, labels, blank, w=None, off=0, max_labels=1023):
    """every integer output against the float64 twin, exactly; the score's special values; -> (gpu outputs, twin)"""
    tw = A.align_twin(y, lens, labels, blank, w, max_labels=max_labels)
    g = gpu_align(y, lens, labels, blank, w, off)
    o = g["offsets"]
    for s, r in enumerate(tw):
        for name in ("frame_class", "frame_pos"):
            bad = np.flatnonzero(g[name][:, s] != r[name])
            assert bad.size == 0, f"stream {s}: {name} differs in {bad.size} frames, first t = {bad[0]}: gpu {g[name][bad[0], s]} twin {r[name][bad[0]]}"
        assert g["token_begin"][o[s]:o[s + 1]].tolist() == r["token_begin"].tolist(), f"stream {s}: token_begin"
        assert g["token_end"][o[s]:o[s + 1]].tolist() == r["token_end"].tolist(), f"stream {s}: token_end"
        if r["status"] == A.IDLE:
            assert g["score"][s] == 0.0
        elif r["status"] == A.REJECTED:
            assert g["score"][s] == -np.inf
        else:
            assert np.isfinite(g["score"][s]) or not np.isfinite(A.path_score64(y[:lens[s], s], r["frame_class"][:lens[s]]))
    return g, tw


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. exact
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(A.EXACT_CASES))
def test_exact_cases(name):
    c = A.EXACT_CASES[name]()
    g, tw = check_exact(c["y"], c["lens"], c["labels"], c["blank"], c["w"])
    assert any(r["status"] == A.ALIGNED for r in tw)
    if name == "uniform":
        assert g["frame_class"][:, 0].tolist() == [5, 0, 5, 9] + [0] * 16 and g["frame_class"][:7, 2].tolist() == [1, 0, 1, 0, 1, 0, 1]


@pytest.mark.parametrize("name,off", [("peaked11", 1), ("K65_blank32", 3), ("peaked11_weighted", 5), ("K4097_blank0", 7), ("uniform", 1)])
def test_column_window_with_odd_offset(name, off):
    c = A.EXACT_CASES[name]()
    check_exact(c["y"], c["lens"], c["labels"], c["blank"], c["w"], off=off)


def test_statuses():
    c = A.EXACT_CASES["statuses"]()
    blank = c["blank"]
    g, tw = check_exact(c["y"], c["lens"], c["labels"], blank)
    assert [r["status"] for r in tw] == [1, 0, 2, 2, 2, 2, 1, 1, 1, 1, 1]
    assert (g["frame_class"][:, 6] == blank).all() and (g["frame_class"][150:, 7] == -1).all() and (g["frame_class"][:, 1:6] == -1).all()
    assert g["frame_class"][:39, 8].tolist() == [7, blank] * 19 + [7]
    c = A.EXACT_CASES["statuses_one_frame_short"]()
    g, tw = check_exact(c["y"], c["lens"], c["labels"], blank)
    assert tw[8]["status"] == A.REJECTED and g["score"][8] == -np.inf
    lists = k.alignments_to_lists(g["result"], c["lens"], g["offsets"])
    assert lists[0]["frame_class"] == tw[0]["frame_class"][:200].tolist() and lists[8]["frame_class"] == [] and lists[1]["frame_class"] == []
    assert lists[0]["token_begin"] == tw[0]["token_begin"].tolist() and lists[8]["token_end"] == [-1] * 20


def test_more_labels_than_the_workspace_was_sized_for():
    """the raw C-ABI with a workspace sized for 5 labels: a stream with 9 is rejected on the device, its neighbours are aligned"""
    lib = k.load_library()
    c = A.EXACT_CASES["capacity_9_labels"]()
    y, lens, labels = c["y"], c["lens"], c["labels"]
    T, S, K = y.shape
    yd = torch.from_numpy(y.reshape(T * S, K)).cuda()
    lab, off, _ = k.ctc.pack_labels(labels, yd.device)
    lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
    nbytes = k.ctc_align_workspace_bytes(T, S, 5)
    assert nbytes < k.ctc_align_workspace_bytes(T, S, 40)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    fc = torch.full((T * S,), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((S,), -7.0, device="cuda")
    tot = torch.zeros(5, dtype=torch.float64, device="cuda")
    assert lib.klstm_ctc_align(yd.data_ptr(), T, S, K, K, lens_d.data_ptr(), lab.data_ptr(), off.data_ptr(), 0, None, fc.data_ptr(), None,
                               None, None, sc.data_ptr(), tot.data_ptr(), ws.data_ptr(), nbytes, None) == 0
    torch.cuda.synchronize()
    tw = A.align_twin(y, lens, labels, 0, max_labels=15)               # 8 bytes serve 32 states: the capacity of that workspace is 15
    tw5 = A.align_twin(y, lens, labels, 0, max_labels=5)
    got = fc.cpu().numpy().reshape(T, S)
    assert tw5[1]["status"] == A.REJECTED and tw[1]["status"] == A.ALIGNED
    assert (got[:, 0] == tw[0]["frame_class"]).all() and (got[:, 2] == tw[2]["frame_class"]).all()
    # 9 labels fit the granularity of the workspace (capacity 15): aligned.  17 do not:
    assert (got[:, 1] == tw[1]["frame_class"]).all() and tot.cpu().tolist()[1:3] == [3.0, 0.0]
    c = A.EXACT_CASES["capacity_17_labels"]()
    lab, off, _ = k.ctc.pack_labels(c["labels"], yd.device)
    yd = torch.from_numpy(c["y"].reshape(T * S, K)).cuda()
    tot.zero_()
    assert lib.klstm_ctc_align(yd.data_ptr(), T, S, K, K, lens_d.data_ptr(), lab.data_ptr(), off.data_ptr(), 0, None, fc.data_ptr(), None,
                               None, None, sc.data_ptr(), tot.data_ptr(), ws.data_ptr(), nbytes, None) == 0
    torch.cuda.synchronize()
    tw = A.align_twin(c["y"], lens, c["labels"], 0, max_labels=15)
    got = fc.cpu().numpy().reshape(T, S)
    assert tw[1]["status"] == A.REJECTED and (got[:, 1] == -1).all() and sc.cpu().numpy()[1] == -np.inf
    assert (got[:, 0] == tw[0]["frame_class"]).all() and (got[:, 2] == tw[2]["frame_class"]).all()
    assert tot.cpu().tolist()[1:4] == [2.0, 1.0, 110.0]


def test_padding_and_idle_streams_are_not_read():
    outs = []
    for name in ("zero", "nan", "inf", "huge"):
        c = A.EXACT_CASES[f"padding_{name}"]()
        g, tw = check_exact(c["y"], c["lens"], c["labels"], 0, w=c["w"])
        assert [r["status"] for r in tw] == [1, 0, 1, 1, 1, 2]
        outs.append([g[n].tobytes() for n in ("frame_class", "frame_pos", "token_begin", "token_end", "score")])
    assert all(o == outs[0] for o in outs[1:])


@pytest.mark.parametrize("name", ["peaked11", "peaked12", "peaked11_weighted", "S32", "L255", "K4097_blank0"])
def test_uncorrupted_peaked_cases_equal_the_greedy_decoder(name):
    """if the unconstrained best path collapses to the labels it is the constrained optimum as well"""
    c = A.EXACT_CASES[name]()
    y, lens = c["y"], c["lens"]
    T, S, K = y.shape
    yd = torch.from_numpy(np.ascontiguousarray(y).reshape(T * S, K)).cuda()
    wd = None if c["w"] is None else torch.from_numpy(c["w"]).cuda()
    dec = k.ctc_greedy_decode(yd, lens, blank=c["blank"], class_weight=wd, refs=c["labels"])
    ali = k.ctc_align(yd, lens, c["labels"], blank=c["blank"], class_weight=wd)
    torch.cuda.synchronize()
    assert all(e in (0, -1) for e in dec.errors.cpu().tolist()), "the case is not peaked on an alignment of its labels"
    assert dec.frame_class.cpu().numpy().tobytes() == ali.frame_class.cpu().numpy().tobytes()


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. optimality on arbitrary posteriors
# ---------------------------------------------------------------------------------------------------------------------------------
def optimality(shape_name, cases):
    """cases: list of (y, lens, labels) of one shape (the seeds).  Bars from the stock fp32 chain over all of them first."""
    twins, worst32 = [], 0.0
    for y, lens, labels in cases:
        t64 = A.align_twin(y, lens, labels, 0)
        t32 = A.align_twin(y, lens, labels, 0, dtype=np.float32)
        twins.append(t64)
        for s, (a, b) in enumerate(zip(t64, t32)):
            if a["status"] == A.ALIGNED:
                n = lens[s]
                worst32 = max(worst32, a["best"] - A.path_score64(y[:n, s], b["frame_class"][:n]))
    n_aligned = 0
    for (y, lens, labels), t64 in zip(cases, twins):
        g = gpu_align(y, lens, labels, 0)
        o = g["offsets"]
        for s, r in enumerate(t64):
            n = lens[s]
            if r["status"] != A.ALIGNED:
                assert (g["frame_class"][:, s] == -1).all() and g["score"][s] == (-np.inf if r["status"] == A.REJECTED else 0.0)
                continue
            n_aligned += 1
            A.validate(g["frame_class"][:n, s], g["frame_pos"][:n, s], g["token_begin"][o[s]:o[s + 1]], g["token_end"][o[s]:o[s + 1]], labels[s], 0)
            assert (g["frame_class"][n:, s] == -1).all() and (g["frame_pos"][n:, s] == -1).all()
            short = r["best"] - A.path_score64(y[:n, s], g["frame_class"][:n, s])
            bar = max(np.sqrt(n) * float(np.spacing(np.float32(abs(r["best"])))), 2.0 * worst32)
            differ = int((g["frame_class"][:n, s] != r["frame_class"][:n]).sum())
            print(f"ctc align {shape_name} len {n} L {len(labels[s])}: shortfall {short:.3g} nats, bar {bar:.3g} (stock fp32 worst {worst32:.3g}), "
                  f"{differ} frames off the float64 path", flush=True)
            bound(short, bar, f"shortfall of the path's float64 score, nats ({shape_name})")
    assert n_aligned >= len(cases)


@pytest.mark.parametrize("K", [29, 48, 512])
@pytest.mark.parametrize("scale", [0.05, 0.2, 1.0, 3.0, 6.0])
def test_optimality_ragged(K, scale):
    cases = []
    for seed in range(4):
        y, labels = R.make_case(100 * seed + K, 300, K, scale, LENS_A, LABS_A)
        cases.append((y.numpy(), LENS_A, labels))
    optimality(f"ragged K={K} scale={scale}", cases)


@pytest.mark.parametrize("T,L", [(8000, 900), (8000, 1023), (16000, 400)])
@pytest.mark.parametrize("scale", [1.0, 3.0])
def test_optimality_long_utterances(T, L, scale):
    cases = []
    for seed in range(4):
        y, labels = R.make_case(1000 * seed + L, T, 29, scale, [T], [L])
        cases.append((y.numpy(), [T], labels))
    optimality(f"long T={T} L={L} scale={scale}", cases)


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. the score
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,T,K,scale", [(1, 300, 48, 3.0), (2, 120, 4097, 8.0), (3, 2000, 29, 1.0)])
def test_score_against_float64(seed, T, K, scale):
    """utterance-length streams only: at a handful of frames float32 summation is nearly exact and the yardstick says nothing"""
    lens = [T, T - 1, (3 * T) // 4, T // 2]
    y, labels = R.make_case(seed, T, K, scale, lens, [20, 20, 15, 0])
    y = y.numpy()
    g = gpu_align(y, lens, labels, 0)
    fc = g["frame_class"]
    assert (fc[0] >= 0).all()
    want = D.path_logp64(y, lens, fc)
    stock = D.path_logp32_stock(y, lens, fc).astype(np.float64)
    got = g["score"].astype(np.float64)
    e_gpu = float(np.max(np.abs(got - want) / np.abs(want)))
    e_32 = float(np.max(np.abs(stock - want) / np.abs(want)))
    print(f"ctc align score T={T} K={K}: gpu {e_gpu:.3g} stock-fp32 {e_32:.3g}", flush=True)
    bound(e_gpu, e_32, "score rel vs fp64 along the returned path (bar: stock fp32 log + sequential sum)")


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. determinism
# ---------------------------------------------------------------------------------------------------------------------------------
def outputs(g):
    return [g[n].tobytes() for n in ("frame_class", "frame_pos", "token_begin", "token_end", "score")]


def test_bit_identical_runs_and_totals():
    y, labels = R.make_case(11, 300, 48, 3.0, LENS_A, LABS_A)
    y = y.numpy()
    totals = torch.zeros(5, dtype=torch.float64, device="cuda")
    g1 = gpu_align(y, LENS_A, labels, 0, totals=totals)
    g2 = gpu_align(y, LENS_A, labels, 0, totals=totals)
    assert outputs(g1) == outputs(g2)
    tw = A.align_twin(y, LENS_A, labels, 0)
    ok = [r["status"] == A.ALIGNED for r in tw]
    once = 0.0
    for s in range(len(LENS_A)):                                         # streams in order
        if ok[s]:
            once += float(g1["score"][s])
    frames = sum(n for n, a in zip(LENS_A, ok) if a)
    blanks = sum(int((g1["frame_pos"][:n, s] == -1).sum()) for s, (n, a) in enumerate(zip(LENS_A, ok)) if a)
    rejected = sum(r["status"] == A.REJECTED for r in tw)
    assert 0 < sum(ok) and blanks > 0
    assert totals.cpu().tolist() == [once + once, 2.0 * sum(ok), 2.0 * rejected, 2.0 * frames, 2.0 * blanks]


def test_an_utterance_does_not_depend_on_its_stream_or_neighbours():
    y1, lab1 = R.make_case(21, 700, 48, 2.0, [700], [150])
    y1 = y1.numpy()
    g1 = gpu_align(y1, [700], lab1, 0)
    lens = [900 - (41 * s) % 500 for s in range(32)]                     # longer neighbours with more labels: another geometry
    lens[17] = 700
    y32, lab32 = R.make_case(22, 900, 48, 2.0, lens, [10 + (37 * s) % 400 for s in range(32)])
    y32 = y32.numpy()
    y32[:700, 17] = y1[:, 0]
    y32[700:, 17] = np.nan
    lab32[17] = lab1[0]
    g32 = gpu_align(y32, lens, lab32, 0)
    o = g32["offsets"]
    assert g32["frame_class"][:700, 17].tobytes() == g1["frame_class"][:, 0].tobytes() and (g32["frame_class"][700:, 17] == -1).all()
    assert g32["frame_pos"][:700, 17].tobytes() == g1["frame_pos"][:, 0].tobytes()
    assert g32["token_begin"][o[17]:o[18]].tobytes() == g1["token_begin"].tobytes()
    assert g32["token_end"][o[17]:o[18]].tobytes() == g1["token_end"].tobytes()
    assert g32["score"][17:18].tobytes() == g1["score"].tobytes()


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_limits_are_refused():
    lib = k.load_library()
    y = torch.full((4, 8), 0.125, device="cuda")
    for blank in (8, -1):
        with pytest.raises(k.KlstmError) as ei:
            k.ctc_align(y, [1, 1, 1, 1], [[], [], [], []], blank=blank)
        assert ei.value.status == 1
    nbytes = k.ctc_align_workspace_bytes(1, 4, 1)
    ws = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
    lens = torch.ones(4, dtype=torch.int32, device="cuda")
    lab = torch.zeros(1, dtype=torch.int32, device="cuda")
    off = torch.zeros(5, dtype=torch.int32, device="cuda")
    fc = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    tb = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((4,), -7.0, device="cuda")

    def call(K, stride, blank, nbytes, tbp=None, tep=None, wsp=ws.data_ptr()):
        return lib.klstm_ctc_align(y.data_ptr(), 1, 4, K, stride, lens.data_ptr(), lab.data_ptr(), off.data_ptr(), blank, None, fc.data_ptr(),
                                   None, tbp, tep, sc.data_ptr(), None, wsp, nbytes, None)
    assert call(1, 8, 0, nbytes) == 2 and b"K" in lib.klstm_last_error()
    assert call(32769, 32769, 0, nbytes) == 2 and b"32768" in lib.klstm_last_error()
    assert call(8, 8, 0, nbytes, tbp=tb.data_ptr()) == 1 and b"together" in lib.klstm_last_error()
    assert call(8, 8, 8, nbytes) == 1 and call(8, 8, -1, nbytes) == 1
    assert call(8, 4, 0, nbytes) == 1                                    # a row stride below K
    assert call(8, 8, 0, nbytes, wsp=ws.data_ptr() + 4) == 1 and b"aligned" in lib.klstm_last_error()
    assert call(8, 8, 0, nbytes - 1) == 1 and b"workspace" in lib.klstm_last_error()
    torch.cuda.synchronize()
    assert bool((fc == -7).all()) and bool((sc == -7.0).all()) and bool((tb == -7).all()), "a refused call wrote an output"
    assert call(8, 8, 0, nbytes) == 0                                    # ... and the same call within the limits runs
    torch.cuda.synchronize()
    assert fc.cpu().tolist() == [0, 0, 0, 0] and np.allclose(sc.cpu().numpy(), np.log(0.125))


# ---------------------------------------------------------------------------------------------------------------------------------
# 10. end to end through the C++ classes (include/klstm_nnet.hpp CtcAligner, AlignCtcWholeUtterances, SetTargetsFromAlignment)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_cpp_train_align_and_train_on_the_alignment():
    """The pattern task of tests/cpp/ctc_decode_test, trained with CTC until the bidirectional net recognises every utterance; all of
    them aligned; alignments against labels, greedy path and greedy score; targets from the alignment; a fresh unidirectional net
    through the frame-level trainer on those targets.  How far a unidirectional net gets on the peaky targets of a CTC model is not
    asserted (only that the loss falls); the figures are printed."""
    from tests.test_ctc_align import run_driver
    r = run_driver("train")
    kv = dict(f.split("=") for f in r.stdout.split() if "=" in f)
    print("ctc_align_test train:", r.stdout.strip(), flush=True)
    print(r.stderr[-3000:], flush=True)
    assert float(kv["ter"]) == 0.0
    assert int(kv["aligned"]) == 12 and int(kv["num_aligned"]) == 12 and int(kv["rejected"]) == 0 and int(kv["skipped"]) == 1
    assert int(kv["collapse_ok"]) == 12 and int(kv["bounds_ok"]) == 12
    assert int(kv["score_ok"]) == 12                                     # no alignment scores above the unconstrained best path
    assert int(kv["greedy_correct"]) == 12 and int(kv["same_as_greedy"]) == 12
    assert int(kv["filled"]) == 12 and int(kv["targets_ok"]) == 12 and int(kv["fl_done"]) == 12
    assert float(kv["fl_last_loss"]) < float(kv["fl_first_loss"])
    assert abs(float(kv["blank_share"]) - float(kv["blank_ratio"])) < 1e-5
