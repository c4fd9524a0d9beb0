"""klstm_ctc_mbr_eval on the device (kaldi_lstm_amd.ctc_mbr_eval) against the float64 composition of torch.nn.functional.ctc_loss on the
CPU (tests/ctc_mbr_ref.py).

Bars (those of tests/test_ctc_gpu.py; the yardstick is "stock fp32", the same composition with losses, gamma and weights all in
float32, ON THE SAME INPUT -- never the kernel):
  diff      max |gpu - fp64| over the valid rows of the counted streams <= 1/8 of max |stock fp32 - fp64| over the same rows
  risk      max |gpu - fp64| over the counted streams <= that of stock fp32
  hyp_logp  max relative error over the listed entries <= that of stock fp32
Conditions every parity case asserts on its own inputs: at least two streams whose listed costs are not all equal, and a stock fp32
diff error above 1e-6.  Which entries are dropped and which streams are idle / rejected / skipped is decided here from lengths and
labels (ctc_mbr_ref.statuses)."""
import functools

import numpy as np
import pytest
import torch

import kaldi_lstm_amd as k
from tests import ctc_mbr_ref as M
from tests.margins import bound

pytestmark = pytest.mark.gpu

# name: seed, T, K, lens, reference lengths, blank, n-best, label capacity (one per chain geometry: 41 / 201 / 401 / 1201 states)
CASES = {"base": (1, 120, 24, [120, 97, 61], [12, 9, 7], 0, 8, 20),
         "ragged": (2, 300, 48, [300, 180, 250, 299, 120, 61, 300, 200], [60, 30, 45, 50, 20, 10, 55, 35], 0, 8, 100),
         "wide": (3, 300, 4096, [300, 290, 200, 150], [50, 60, 30, 20], 0, 4, 200),
         "long": (14, 700, 64, [700, 650], [250, 200], 0, 2, 600),
         "odd": (5, 120, 23, [120, 97, 61], [12, 9, 7], 22, 8, 20)}
RAGGED_COUNTS = [8, 3, 8, 5, 1, 8, 2, 8]


@functools.lru_cache(maxsize=None)
def case(name):
    seed, T, K, lens, ref_lens, blank, nbest, max_len = CASES[name]
    c = M.make_case(seed, T, K, lens, ref_lens, blank=blank, nbest=nbest)
    if name == "ragged":
        c["counts"] = list(RAGGED_COUNTS)
        c["lists"] = [l[:n] for l, n in zip(c["lists"], c["counts"])]
        c["costs"] = [w[:n] for w, n in zip(c["costs"], c["counts"])]
    c.update(T=T, K=K, lens=lens, blank=blank, N=nbest, max_len=max_len)
    return c


@functools.lru_cache(maxsize=None)
def case_parts(name, dtype):
    c = case(name)
    return M.parts(c["y"], c["lens"], c["lists"], c["refs"], c["blank"], dtype)


def list_arrays(lists, costs, counts, N, stride, garbage=False):
    """the beam search's device arrays from Python lists; garbage: what no call may read (slots q >= count) is filled with nonsense"""
    S = len(lists)
    hyp = np.full((S, N, stride), 10 ** 6 if garbage else 0, np.int32)
    hyp_len = np.full((S, N), -7 if garbage else 0, np.int32)
    errors = np.full((S, N), -1, np.int32)
    for s in range(S):
        for q, lab in enumerate(lists[s]):
            hyp[s, q, :len(lab)] = lab
            hyp_len[s, q] = len(lab)
            errors[s, q] = costs[s][q]
    return tuple(torch.from_numpy(a).cuda() for a in (hyp, hyp_len, np.asarray(counts, np.int32), errors))


def gpu_mbr(y, lens, arrays, refs, blank, kappa, lam, max_len, pad=0, off=0, totals=None):
    """y [T, S, K] CPU float32 -> dict of numpy outputs; pad > 0: both matrices are column windows (offset `off`) of wider ones"""
    T, S, K = y.shape
    if pad:
        yw = torch.full((T * S, K + pad), 7.0, device="cuda")
        yw[:, off:off + K] = y.reshape(T * S, K).cuda()
        yd = yw[:, off:off + K]
        dw = torch.full((T * S, K + 2 * pad), 5.0, device="cuda")
        dd = dw[:, off:off + K]
    else:
        yd, dd = y.reshape(T * S, K).cuda().contiguous(), torch.full((T * S, K), 5.0, device="cuda")
    y0 = yd.clone()
    r = k.ctc_mbr_eval(yd, lens, arrays, refs=refs if lam > 0 else None, blank=blank, risk_scale=kappa, ctc_weight=lam, max_len=max_len,
                       diff=dd, totals=totals)
    torch.cuda.synchronize()
    assert torch.equal(yd.view(torch.int32), y0.view(torch.int32)), "the posterior matrix was modified"
    out = dict(risk=r.risk.cpu().numpy(), diff=r.diff.cpu().numpy().reshape(T, S, K), logp=r.hyp_logp.cpu().numpy(),
               post=r.hyp_post.cpu().numpy(), ref_loss=None if r.ref_loss is None else r.ref_loss.cpu().numpy())
    if pad:
        dw[:, off:off + K] = 5.0
        yw[:, off:off + K] = 7.0
        assert bool((dw == 5.0).all()) and bool((yw == 7.0).all()), "columns outside the window were touched"
    return out


def check_outputs(c, out, o64, o32, status, dropped, kappa, lam, totals=None):
    """the bars and the exact relations of one call; o64 / o32: compose() over the counted streams with the dropped entries taken out"""
    y, lens, K, N = c["y"], c["lens"], c["K"], c["N"]
    S = len(lens)
    e_gpu = e_32 = r_gpu = r_32 = l_gpu = l_32 = 0.0
    lam32 = np.float32(lam)
    for s in range(S):
        n = max(min(lens[s], c["T"]), 0)
        if status[s] != "counted":
            assert not out["diff"][:, s].any(), f"stream {s} ({status[s]}): diff rows are not exactly zero"
            assert out["risk"][s] == (0.0 if status[s] == "idle" else -1.0) and not out["post"][s].any()
            continue
        assert not out["diff"][n:, s].any(), f"stream {s}: padding rows are not exactly zero"
        live = [q for q in range(c["counts"][s]) if not dropped[s][q]]
        dead = [q for q in range(N) if q not in live]
        assert np.isneginf(out["logp"][s, dead]).all() and not out["post"][s, dead].any()
        d = out["diff"][:n, s].astype(np.float64)
        e_gpu = max(e_gpu, float(np.abs(d - o64["diff"][:n, s]).max()))
        e_32 = max(e_32, float(np.abs(o32["diff"][:n, s] - o64["diff"][:n, s]).max()))
        r_gpu = max(r_gpu, abs(float(out["risk"][s]) - o64["risk"][s]))
        r_32 = max(r_32, abs(o32["risk"][s] - o64["risk"][s]))
        l64, l32 = np.array(o64["logp"][s]), np.array(o32["logp"][s])
        l_gpu = max(l_gpu, float(np.abs((out["logp"][s, live] - l64) / l64).max()))
        l_32 = max(l_32, float(np.abs((l32 - l64) / l64).max()))
        bound(abs(float(out["post"][s].astype(np.float64).sum()) - 1.0), 1e-6, "sum_q post - 1")
        # the risk part sums to zero over the classes of a row
        ys = y[:n, s].double().sum(-1).numpy()
        wmax = max(c["costs"][s][q] for q in live)
        bound(float(np.abs(d.sum(-1) - lam * (ys - 1.0)).max()), K * 2.0 ** -23 * (1 + kappa * wmax), "sum_k diff - lam (sum_k y - 1)")
        # columns of classes in no labelling: lam * y, rounded once
        used = {c["blank"]} | {v for q in live for v in c["lists"][s][q]} | (set(c["refs"][s]) if lam > 0 else set())
        free = [v for v in range(K) if v not in used]
        want = (lam32 * y[:n, s].numpy()[:, free]).astype(np.float32) if lam > 0 else np.zeros((n, len(free)), np.float32)
        assert out["diff"][:n, s][:, free].tobytes() == want.tobytes(), f"stream {s}: a column of no labelling is not lam * y"
        if lam > 0:
            assert np.isfinite(out["ref_loss"][s]) and abs(out["ref_loss"][s] - o64["ref_loss"][s]) <= 1e-5 * o64["ref_loss"][s]
    print(f"mbr T={c['T']} S={S} K={K} N={N} kappa={kappa} lam={lam}: diff gpu {e_gpu:.3g} stock {e_32:.3g} | risk gpu {r_gpu:.3g} stock "
          f"{r_32:.3g} | logp gpu {l_gpu:.3g} stock {l_32:.3g}", flush=True)
    counted = [s for s in range(S) if status[s] == "counted"]
    assert sum(len(set(c["costs"][s])) > 1 for s in counted) >= 2, "fewer than two streams with unequal costs"
    assert e_32 > 1e-6, "stock fp32 is too close to float64 on this input for the bar to mean anything"
    bound(e_gpu, e_32 / 8.0, "diff vs fp64 (bar: stock fp32 / 8)")
    bound(r_gpu, r_32, "risk vs fp64 (bar: stock fp32)")
    bound(l_gpu, l_32, "hyp_logp rel vs fp64 (bar: stock fp32)")
    if totals is not None:
        tot = totals.cpu().numpy()
        assert tot[0] == sum(float(out["risk"][s]) for s in counted) and tot[1] == sum(c["costs"][s][0] for s in counted)
        assert tot[2] == len(counted) and tot[3] == sum(st in ("rejected", "skipped") for st in status)
        assert tot[4] == sum(lens[s] for s in counted)
        assert tot[5] == (sum(float(out["ref_loss"][s]) for s in counted) if lam > 0 else 0.0)


def check_case(name, kappa, lam, pad=0, off=0, max_len=None):
    c = case(name)
    T, K, lens, N = c["T"], c["K"], c["lens"], c["N"]
    max_len = max_len or c["max_len"]
    status, dropped = M.statuses(lens, c["lists"], c["costs"], c["counts"], c["refs"], K, c["blank"], T, N, max_len, lam)
    assert all(st == "counted" for st in status) and not any(any(d) for d in dropped)
    o64 = M.compose(case_parts(name, torch.float64), c["costs"], kappa, lam, T, K)
    o32 = M.compose(case_parts(name, torch.float32), c["costs"], kappa, lam, T, K)
    totals = torch.zeros(6, dtype=torch.float64, device="cuda")
    arrays = list_arrays(c["lists"], c["costs"], c["counts"], N, T, garbage=True)
    out = gpu_mbr(c["y"], lens, arrays, c["refs"], c["blank"], kappa, lam, max_len, pad, off, totals)
    check_outputs(c, out, o64, o32, status, dropped, kappa, lam, totals)
    return out


@pytest.mark.parametrize("lam", [0.0, 0.3])
@pytest.mark.parametrize("name,kappa", [("base", 1.0), ("ragged", 0.5), ("wide", 1.0), ("long", 0.5)])
def test_parity(name, kappa, lam):
    check_case(name, kappa, lam)


def test_parity_sixteen_waves_one_state():
    """label capacity 400: the chain of 16 waves with one state per thread, on the base case"""
    a = check_case("base", 1.0, 0.3, max_len=400)
    b = check_case("base", 1.0, 0.3)
    assert a["diff"].tobytes() == b["diff"].tobytes() and a["logp"].tobytes() == b["logp"].tobytes()      # the geometry changes no bit


@pytest.mark.parametrize("lam", [0.0, 0.3])
def test_parity_odd_k_last_blank_column_window(lam):
    """K = 23, blank = K - 1, both matrices column windows at an odd offset of wider ones: the scalar path, pad columns untouched"""
    check_case("odd", 1.0, lam, pad=9, off=3)


def test_parity_vector_path_in_a_window():
    check_case("ragged", 1.0, 0.3, pad=16, off=0)              # rows stay 16-byte aligned: float4 with a stride


def test_exact_relations_with_ctc_eval():
    c = case("ragged")
    T, K, lens, N = c["T"], c["K"], c["lens"], c["N"]
    arrays = list_arrays(c["lists"], c["costs"], c["counts"], N, T)
    out = gpu_mbr(c["y"], lens, arrays, c["refs"], 0, 1.0, 0.3, c["max_len"])
    yd = c["y"].reshape(T * len(lens), K).cuda()
    for q in range(N):
        listed = [s for s in range(len(lens)) if q < c["counts"][s]]
        labels = [c["lists"][s][q] if s in listed else [] for s in range(len(lens))]
        loss, _ = k.ctc_eval(yd, lens, labels, blank=0)
        loss = loss.cpu().numpy()
        assert (-loss[listed]).tobytes() == out["logp"][listed, q].tobytes(), f"entry {q}: hyp_logp is not -utt_loss of klstm_ctc_eval"
    loss, _ = k.ctc_eval(yd, lens, c["refs"], blank=0)
    assert loss.cpu().numpy().tobytes() == out["ref_loss"].tobytes()


def test_single_entry_without_ctc_term_is_exactly_zero():
    c = case("base")
    arrays = list_arrays([l[:1] for l in c["lists"]], [w[:1] for w in c["costs"]], [1, 1, 1], 1, c["T"])
    out = gpu_mbr(c["y"], c["lens"], arrays, None, 0, 1.0, 0.0, c["max_len"])
    assert not out["diff"].any() and (out["post"] == 1.0).all()
    assert out["risk"].tolist() == [float(w[0]) for w in c["costs"]]


def planted():
    """the ragged case with every status planted; -> (case dict, garbage-free copy of stream 0's list)"""
    c = dict(case("ragged"))
    K, lens = c["K"], list(c["lens"])
    lists, costs = [[list(h) for h in l] for l in case("ragged")["lists"]], [list(w) for w in case("ragged")["costs"]]
    full = M.make_case(*CASES["ragged"][:5], blank=0, nbest=8)
    lists[1], costs[1] = [list(h) for h in full["lists"][1][:6]], list(full["costs"][1][:6])
    lists[1][2] = [1 + j % 7 for j in range(101)]                  # longer than the capacity of 100
    lists[1][3][2] = 0                                             # a blank inside
    lists[1][4] = [5] * (lens[1] // 2 + 1)                         # 91 equal labels need 181 frames, the stream has 180
    costs[2][1] = -1                                               # the beam's "not counted": skipped
    lists[3], costs[3] = [[3, 0, 4], [K, 2]], [1, 2]               # every entry dropped: skipped
    refs = [list(r) for r in c["refs"]]
    refs[4][1] = K                                                 # a reference klstm_ctc_eval rejects
    lens[5] = 0                                                    # idle
    counts = [len(l) for l in lists]
    counts[6] = 9                                                  # outside [0, N]: rejected
    c.update(lens=lens, lists=lists, costs=costs, counts=counts, refs=refs)
    return c


def test_statuses_garbage_and_unread_rows():
    c = planted()
    T, K, lens, N, lam, kappa = c["T"], c["K"], c["lens"], c["N"], 0.3, 1.0
    S = len(lens)
    status, dropped = M.statuses(lens, c["lists"], c["costs"], c["counts"], c["refs"], K, 0, T, N, c["max_len"], lam)
    assert status == ["counted", "counted", "skipped", "skipped", "rejected", "idle", "rejected", "counted"]
    assert dropped[1] == [False, False, True, True, True, False]
    keep = [[q for q in range(len(dropped[s])) if not dropped[s][q]] if status[s] == "counted" else [] for s in range(S)]
    live_lists = [[c["lists"][s][q] for q in keep[s]] for s in range(S)]
    live_costs = [[c["costs"][s][q] for q in keep[s]] for s in range(S)]
    o64, o32 = (M.compose(M.parts(c["y"], lens, live_lists, c["refs"], 0, dt, streams=[0, 1, 7]), live_costs, kappa, lam, T, K)
                for dt in (torch.float64, torch.float32))
    lists6 = [l[:8] for l in c["lists"]]                           # stream 6 says 9 entries and has room for 8
    totals = torch.zeros(6, dtype=torch.float64, device="cuda")
    a = gpu_mbr(c["y"], lens, list_arrays(lists6, c["costs"], c["counts"], N, T), c["refs"], 0, kappa, lam, c["max_len"], totals=totals)
    check_outputs(c, a, o64, o32, status, dropped, kappa, lam, totals)
    # nonsense in the slots beyond count, NaN in every row that is not to be read: the same bits
    y = c["y"].clone()
    for s in range(S):
        y[lens[s] if status[s] == "counted" else 0:, s] = float("nan")
    b = gpu_mbr(y, lens, list_arrays(lists6, c["costs"], c["counts"], N, T, garbage=True), c["refs"], 0, kappa, lam, c["max_len"])
    for key in ("risk", "diff", "logp", "post", "ref_loss"):
        assert a[key].tobytes() == b[key].tobytes(), key


def test_bit_identical_runs_and_stream_permutation():
    c = case("ragged")
    T, lens, N = c["T"], c["lens"], c["N"]

    def run(perm):
        arrays = list_arrays([c["lists"][p] for p in perm], [c["costs"][p] for p in perm], [c["counts"][p] for p in perm], N, T)
        return gpu_mbr(c["y"][:, perm].contiguous(), [lens[p] for p in perm], arrays, [c["refs"][p] for p in perm], 0, 0.5, 0.3, c["max_len"])
    ident = list(range(len(lens)))
    a, b = run(ident), run(ident)
    for key in ("risk", "diff", "logp", "post", "ref_loss"):
        assert a[key].tobytes() == b[key].tobytes(), key
    perm = [3, 7, 0, 5, 1, 6, 2, 4]
    p = run(perm)
    for key in ("risk", "logp", "post", "ref_loss"):
        assert p[key].tobytes() == np.ascontiguousarray(a[key][perm]).tobytes(), key
    assert p["diff"].tobytes() == np.ascontiguousarray(a["diff"][:, perm]).tobytes()


def test_refusals():
    lib = k.load_library()
    T, S, K, N, L = 6, 2, 8, 2, 4
    y = torch.full((T * S, K), 0.125, device="cuda")
    d = torch.full((T * S, K), 5.0, device="cuda")
    lens = torch.full((S,), T, dtype=torch.int32, device="cuda")
    hyp, hyp_len, cnt, err = list_arrays([[[1, 2], [1]]] * S, [[0, 1]] * S, [2] * S, N, T)
    lab, off, _ = k.ctc.pack_labels([[1, 2]] * S, y.device)
    risk = torch.full((S,), 9.0, device="cuda")
    ws = torch.empty(k.ctc_mbr_workspace_bytes(T, S, N, L, True), dtype=torch.uint8, device="cuda")

    def call(**kw):
        a = dict(net_out=y.data_ptr(), T=T, S=S, K=K, stride=K, lens=lens.data_ptr(), blank=0, hyp=hyp.data_ptr(), hstride=T,
                 hyp_len=hyp_len.data_ptr(), cnt=cnt.data_ptr(), err=err.data_ptr(), N=N, lab=lab.data_ptr(), off=off.data_ptr(), kappa=1.0,
                 lam=0.5, diff=d.data_ptr(), dstride=K, risk=risk.data_ptr(), logp=None, post=None, rl=None, tot=None, ws=ws.data_ptr(),
                 nbytes=ws.numel(), stream=None)
        a.update(kw)
        return lib.klstm_ctc_mbr_eval(*a.values()), lib.klstm_last_error()
    nan = float("nan")
    bad = [dict(net_out=None), dict(lens=None), dict(hyp=None), dict(hyp_len=None), dict(cnt=None), dict(err=None), dict(diff=None),
           dict(risk=None), dict(ws=None), dict(lab=None), dict(off=None), dict(lab=None, off=None), dict(lam=0.0),
           dict(diff=y.data_ptr()), dict(kappa=0.0), dict(kappa=-1.0), dict(kappa=nan), dict(kappa=float("inf")), dict(lam=-0.5), dict(lam=nan),
           dict(hstride=0), dict(blank=K), dict(stride=K - 1), dict(nbytes=k.ctc_mbr_workspace_bytes(T, S, N, 0, True) - 1)]
    for kw in bad:
        st, msg = call(**kw)
        assert st == 1 and msg.startswith(b"klstm_ctc_mbr_eval"), (kw, st, msg)
    for kw in (dict(N=17), dict(S=33), dict(K=32769, stride=32769, dstride=32769), dict(K=1, stride=1, dstride=1)):
        st, msg = call(**kw)
        assert st == 2 and msg.startswith(b"klstm_ctc_mbr_eval"), (kw, st, msg)
    with pytest.raises(k.KlstmError) as ei:
        k.ctc_mbr_workspace_bytes(T, S, N, 1024)
    assert ei.value.status == 2
    torch.cuda.synchronize()
    assert bool((d == 5.0).all()) and bool((risk == 9.0).all()), "a refused call launched something"
    st, _ = call()
    torch.cuda.synchronize()
    assert st == 0 and bool((risk >= 0).all())                      # and the same arguments, unbroken, are taken


def test_limit_frames_and_labels():
    """T = 2047, S = 2, two entries and the reference, 1023 labels on one stream: 16 waves with two states per thread, 0.2 GB"""
    T, K, lens = 2047, 64, [2047, 1500]
    refs = M.random_refs(21, K, [1023, 400], no_repeats=True)
    y = M.peaked(21, T, K, lens, refs)
    lists = [[list(r), list(r)] for r in refs]
    for s in range(2):
        j = len(refs[s]) // 2
        lists[s][1][j] = next(v for v in range(1, K) if v not in (lists[s][1][j - 1], lists[s][1][j], lists[s][1][j + 1]))
    costs = [[0, 1], [0, 1]]
    c = dict(y=y, refs=refs, lists=lists, costs=costs, counts=[2, 2], T=T, K=K, lens=lens, blank=0, N=2, max_len=1023)
    status, dropped = M.statuses(lens, lists, costs, [2, 2], refs, K, 0, T, 2, 1023, 0.3)
    assert status == ["counted", "counted"] and not any(any(d) for d in dropped)
    assert k.ctc_mbr_workspace_bytes(T, 2, 2, 1023, True) < 0.25 * 2 ** 30
    o64, o32 = (M.compose(M.parts(y, lens, lists, refs, 0, dt), costs, 1.0, 0.3, T, K) for dt in (torch.float64, torch.float32))
    totals = torch.zeros(6, dtype=torch.float64, device="cuda")
    out = gpu_mbr(y, lens, list_arrays(lists, costs, [2, 2], 2, T), refs, 0, 1.0, 0.3, 1023, totals=totals)
    check_outputs(c, out, o64, o32, status, dropped, 1.0, 0.3, totals)


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end through the C++ classes (include/klstm_nnet.hpp CtcMbr, TrainMbrWholeUtterances; tests/cpp/ctc_mbr_test.cpp)
# ---------------------------------------------------------------------------------------------------------------------------------
# CTC epochs before the risk training (so few that the 1-best still makes errors: asserted) and its learning rate, per kind of net
SCHEDULE = {"blstm": (20, 0.01), "lstm": (50, 0.01)}


@pytest.mark.parametrize("kind", ["blstm", "lstm"])
def test_cpp_trainer_lowers_the_risk(kind, tmp_path):
    from tests.test_ctc_mbr import run_driver
    dump = str(tmp_path / "dump.bin")
    epochs, lr = SCHEDULE[kind]
    r = run_driver("train", kind, dump, epochs, lr)
    kv = dict(f.split("=") for f in r.stdout.split() if "=" in f)
    print(f"ctc_mbr_test train {kind}:", r.stdout.strip(), flush=True)
    assert float(kv["ter_before"]) > 0, "the net was trained until its 1-best had no errors left: nothing to minimise"
    assert float(kv["risk_after"]) < float(kv["risk_before"]), (kv["risk_before"], kv["risk_after"])
    assert int(kv["skipped"]) == 1 and int(kv["done"]) == 12
    # the minibatch the driver dumped (its second: the objects had been through another shape): Python's path gives the same bits
    raw = np.fromfile(dump, dtype=np.int32)
    T, S, K, N, nlab = (int(v) for v in raw[:5])
    p = 5

    def take(n, dtype=np.int32):
        nonlocal p
        a = raw[p:p + n].view(dtype)
        p += n
        return a
    lens, off, flat = take(S).tolist(), take(S + 1).tolist(), take(nlab).tolist()
    cnt, hlen, err, hyp = take(S), take(S * N).reshape(S, N), take(S * N).reshape(S, N), take(S * N * T).reshape(S, N, T)
    post, diff = take(T * S * K, np.float32).reshape(T * S, K), take(T * S * K, np.float32)
    risk, logp = take(S, np.float32), take(S * N, np.float32)
    refs = [flat[off[s]:off[s + 1]] for s in range(S)]
    y = torch.from_numpy(post.copy()).cuda()
    beam = k.ctc_beam_decode(y, lens, blank=0, beam=8, cands=5, nbest=N, refs=refs)
    for got, want in ((beam.nbest_count, cnt), (beam.errors, err)):
        assert got.cpu().numpy().tobytes() == want.tobytes()
    mine = k.ctc_mbr_eval(y, lens, beam, refs=refs, blank=0, risk_scale=1.0, ctc_weight=0.1, max_len=min(1023, 2 * max(map(len, refs)) + 8))
    assert mine.diff.cpu().numpy().tobytes() == diff.tobytes() and mine.risk.cpu().numpy().tobytes() == risk.tobytes()
    assert mine.hyp_logp.cpu().numpy().tobytes() == logp.tobytes()
    assert diff.any() and (risk >= 0).all()
