"""klstm_ctc_eval on the device (kaldi_lstm_amd.ctc_eval) against torch.nn.functional.ctc_loss on the CPU in float64 (tests/ctc_ref.py).

Bars (both relative to what stock fp32 CTC -- the same torch call in float32 -- delivers ON THE SAME INPUT; the yardstick is torch,
never the kernel):
  diff      max |gpu - fp64| over the valid rows of the feasible streams <= 1/8 of max |torch fp32 - fp64| over the same rows.  Entries are
            bounded by 1, so absolute = relative to the largest.  Stock fp32 carries log alpha ~ -1e3 with an ulp of 1e-4; the kernel's
            normalised recursion does not, and the numpy twin of it measures 73 to 1000 times closer to fp64 than stock fp32 on these
            inputs; an eighth leaves the kernel's other summation order and its fast exp / log room, and fails a plain log-domain port.
  utt_loss  max relative error over the feasible streams <= that of torch fp32 on the same input (the offsets are summed in double).
            utt_loss is a float: its own rounding is 6e-8, which is why every case here has utterance-length streams (stock fp32 is
            then off by 3e-7 and more).
Conditions: padding rows and every row of an idle or rejected stream are exactly 0.0; a rejected stream's loss is +inf; the rejected
count equals the one derived from the lengths.  Which streams are infeasible is decided here from the lengths and labels."""
import numpy as np
import pytest
import torch

import kaldi_lstm_amd as k
from tests import ctc_ref as R
from tests.margins import bound

pytestmark = pytest.mark.gpu


def gpu_eval(y, lens, labels, blank, pad=0, totals=None):
    """y [T, S, K] CPU float32 -> (utt_loss [S] numpy, diff [T, S, K] numpy); pad > 0: both matrices are column windows of wider ones"""
    T, S, K = y.shape
    if pad:
        yw = torch.full((T * S, K + pad), 7.0, device="cuda")
        yw[:, :K] = y.reshape(T * S, K).cuda()
        yd = yw[:, :K]
        dw = torch.full((T * S, K + 2 * pad), 5.0, device="cuda")
        dd = dw[:, :K]
    else:
        yd, dd = y.reshape(T * S, K).cuda().contiguous(), torch.full((T * S, K), 5.0, device="cuda")
    y0 = yd.clone()
    loss, diff = k.ctc_eval(yd, lens, labels, blank=blank, diff=dd, totals=totals)
    torch.cuda.synchronize()
    assert torch.equal(yd, y0), "the posterior matrix was modified"
    if pad:
        assert bool((dw[:, K:] == 5.0).all()) and bool((yw[:, K:] == 7.0).all()), "columns beyond K were touched"
    return loss.cpu().numpy(), diff.cpu().numpy().reshape(T, S, K)


def check_case(y, lens, labels, blank=0, pad=0):
    T, S, K = y.shape
    inf = R.infeasible(lens, labels, K, blank)
    l64, d64 = R.oracle(y, lens, labels, blank, torch.float64)
    l32, d32 = R.oracle(y, lens, labels, blank, torch.float32)
    totals = torch.zeros(4, dtype=torch.float64, device="cuda")
    loss, diff = gpu_eval(y, lens, labels, blank, pad, totals)
    e_gpu = e_32 = r_gpu = r_32 = 0.0
    for s in range(S):
        n = lens[s]
        assert not diff[n:, s].any(), f"stream {s}: padding rows are not exactly zero"
        if n == 0:
            assert loss[s] == 0.0
            continue
        if inf[s]:
            assert np.isposinf(loss[s]) and not diff[:, s].any(), f"stream {s} is infeasible: loss {loss[s]}"
            continue
        assert np.isfinite(l64[s]) and np.isfinite(loss[s])
        e_gpu = max(e_gpu, float(np.abs(diff[:n, s].astype(np.float64) - d64[:n, s]).max()))
        e_32 = max(e_32, float(np.abs(d32[:n, s].astype(np.float64) - d64[:n, s]).max()))
        r_gpu = max(r_gpu, abs(float(loss[s]) - l64[s]) / abs(l64[s]))
        r_32 = max(r_32, abs(l32[s] - l64[s]) / abs(l64[s]))
        # consistency: gamma sums to one on every valid frame
        ys = y[:n, s].double().sum(-1).numpy()
        bound(float(np.abs(diff[:n, s].astype(np.float64).sum(-1) - (ys - 1.0)).max()), K * 2.0 ** -23, "sum_k diff - (sum_k y - 1)")
    print(f"ctc case T={T} S={S} K={K}: diff gpu {e_gpu:.3g} torch-fp32 {e_32:.3g} | loss gpu {r_gpu:.3g} torch-fp32 {r_32:.3g}", flush=True)
    bound(e_gpu, e_32 / 8.0, "diff vs fp64 (bar: torch fp32 / 8)")
    bound(r_gpu, r_32, "utt_loss rel vs fp64 (bar: torch fp32)")
    tot = totals.cpu().numpy()
    ok = [s for s in range(S) if lens[s] > 0 and not inf[s]]
    assert tot[1] == len(ok) and tot[2] == sum(inf) and tot[3] == sum(lens[s] for s in ok)
    assert tot[0] == sum(float(loss[s]) for s in ok)           # doubles of floats, added in stream order
    return loss, diff


LENS_A = [300, 299, 250, 180, 120, 61, 30, 7]
LABS_A = [40, 60, 33, 50, 60, 30, 29, 3]


def test_parity_ragged_with_repeats():
    y, labels = R.make_case(1, 300, 48, 3.0, LENS_A, LABS_A, equal_labels=(5,))
    assert not any(R.infeasible(LENS_A, labels, 48, 0))      # stream 5: 30 repeats need 59 frames, it has 61
    check_case(y, LENS_A, labels)


def test_parity_with_infeasible_streams():
    lens = LENS_A[:5] + [58, 30, 2]
    labs = LABS_A[:6] + [31, 3]
    y, labels = R.make_case(1, 300, 48, 3.0, lens, labs, equal_labels=(5,))
    assert R.infeasible(lens, labels, 48, 0) == [False] * 5 + [True] * 3
    check_case(y, lens, labels)


def test_parity_peaked_wide():
    lens, labs = [1000 - 37 * i for i in range(16)], [120 - 5 * i for i in range(16)]
    y, labels = R.make_case(3, 1000, 4096, 8.0, lens, labs)
    assert not any(R.infeasible(lens, labels, 4096, 0))
    check_case(y, lens, labels)


def test_parity_long_flat():
    lens, labs = [1500, 1200, 900, 10], [500, 400, 1, 4]
    y, labels = R.make_case(4, 1500, 64, 1.0, lens, labs)
    assert not any(R.infeasible(lens, labels, 64, 0))
    check_case(y, lens, labels)


def test_limit_streams_frames_labels():
    """S = 32, T = 2047 (T * S = 65504), 1023 labels on one stream: the 16-wave chain with two states per thread, 1.07 GB of workspace"""
    lens = [2047] + [2047 - 61 * i for i in range(1, 32)]
    labs = [1023] + [min((37 * i) % 700 + 1, lens[i] // 3) for i in range(1, 32)]
    lens[7], labs[7] = 0, 0                     # an idle stream among them
    labs[9] = 0                                 # and an empty label sequence
    y, labels = R.make_case(5, 2047, 64, 2.0, lens, labs)
    check_case(y, lens, labels)


def test_limit_classes():
    lens, labs = [100, 93, 100, 41], [30, 12, 49, 20]
    y, labels = R.make_case(6, 100, 32768, 6.0, lens, labs)
    check_case(y, lens, labels)


def test_idle_empty_blank_and_strides():
    """an idle stream, L = 0, a blank that is not class 0, both matrices as column windows of wider ones, K not a multiple of 4"""
    lens, labs = [400, 0, 380, 215, 399], [70, 5, 0, 100, 199]
    y, labels = R.make_case(7, 400, 45, 2.5, lens, labs, blank=17)
    assert all(17 not in lab for lab in labels)
    loss, _ = check_case(y, lens, labels, blank=17, pad=19)
    assert loss[1] == 0.0
    y, labels = R.make_case(8, 400, 48, 2.5, lens, labs, blank=47)
    check_case(y, lens, labels, blank=47, pad=16)               # rows stay 16-byte aligned: the vector path with a stride


def test_out_of_range_label_is_rejected():
    lens, labs = [200, 200, 200], [20, 20, 20]
    y, labels = R.make_case(9, 200, 32, 2.0, lens, labs)
    labels[1][4] = 32                                           # outside [0, K)
    labels[2][0] = 0                                            # the blank itself
    loss, diff = gpu_eval(y, lens, labels, 0)
    assert np.isfinite(loss[0]) and np.isposinf(loss[1]) and np.isposinf(loss[2])
    assert diff[:, 0].any() and not diff[:, 1:].any()


def test_bit_identical_runs_and_stream_permutation():
    lens = LENS_A[:5] + [58, 30, 61]
    y, labels = R.make_case(11, 300, 48, 3.0, lens, LABS_A, equal_labels=(7,))
    l1, d1 = gpu_eval(y, lens, labels, 0)
    l2, d2 = gpu_eval(y, lens, labels, 0)
    assert l1.tobytes() == l2.tobytes() and d1.tobytes() == d2.tobytes()
    perm = [3, 7, 0, 5, 1, 6, 2, 4]
    lp, dp = gpu_eval(y[:, perm].contiguous(), [lens[p] for p in perm], [labels[p] for p in perm], 0)
    assert lp.tobytes() == l1[perm].tobytes()
    assert np.ascontiguousarray(dp).tobytes() == np.ascontiguousarray(d1[:, perm]).tobytes()
    # ... and with fewer neighbours: the first three utterances alone, in a shorter block
    l3, d3 = gpu_eval(y[:, :3].contiguous(), lens[:3], labels[:3], 0)
    assert l3.tobytes() == l1[:3].tobytes() and np.ascontiguousarray(d3).tobytes() == np.ascontiguousarray(d1[:, :3]).tobytes()


def test_limits_are_refused():
    y = torch.full((4, 8), 0.125, device="cuda")
    for T, S, L in ((2048, 32, 10), (10, 33, 10), (10, 4, 1024)):
        with pytest.raises(k.KlstmError) as ei:
            k.ctc_workspace_bytes(T, S, L)
        assert ei.value.status == 2
    with pytest.raises(k.KlstmError):
        k.ctc_eval(y, [1, 1, 1, 1], [[1]] * 4, blank=8)
    lib = k.load_library()
    ws = torch.empty(k.ctc_workspace_bytes(1, 4, 1), dtype=torch.uint8, device="cuda")
    lens = torch.ones(4, dtype=torch.int32, device="cuda")
    lab, off, _ = k.ctc.pack_labels([[1]] * 4, y.device)
    big = torch.empty(1, device="cuda")
    st = lib.klstm_ctc_eval(big.data_ptr(), 1, 4, 32769, 32769, lens.data_ptr(), lab.data_ptr(), off.data_ptr(), 0, big.data_ptr() + 4, 32769,
                            big.data_ptr(), None, ws.data_ptr(), ws.numel(), None)
    assert st == 2 and b"32768" in lib.klstm_last_error()       # refused before anything is launched


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end through the C++ classes (include/klstm_nnet.hpp Ctc, WholeUtteranceBatcher, TrainCtcWholeUtterances; tests/cpp/ctc_test)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_cpp_trainer_bidirectional(tmp_path):
    from tests.test_ctc import run_driver
    dump = str(tmp_path / "dump.bin")
    r = run_driver("train", "blstm", dump)
    kv = dict(f.split("=") for f in r.stdout.split() if "=" in f)
    first, last = float(kv["first_epoch_loss_per_frame"]), float(kv["last_epoch_loss_per_frame"])
    print("ctc_test train blstm:", r.stdout.strip(), flush=True)
    assert last < first, (first, last)
    assert int(kv["rejected"]) == 0 and int(kv["skipped"]) == 0
    # the minibatch the driver dumped: Python's ctc_eval on the same posteriors gives the same bits
    raw = np.fromfile(dump, dtype=np.int32)
    T, S, K, nlab = (int(v) for v in raw[:4])
    p = 4
    lens = raw[p:p + S].tolist(); p += S
    off = raw[p:p + S + 1].tolist(); p += S + 1
    flat = raw[p:p + nlab].tolist(); p += nlab
    post = raw[p:p + T * S * K].view(np.float32).reshape(T * S, K); p += T * S * K
    diff = raw[p:p + T * S * K].view(np.float32).reshape(T * S, K); p += T * S * K
    loss = raw[p:p + S].view(np.float32)
    labels = [flat[off[s]:off[s + 1]] for s in range(S)]
    l2, d2 = k.ctc_eval(torch.from_numpy(post.copy()).cuda(), lens, labels, blank=0)
    assert d2.cpu().numpy().tobytes() == diff.tobytes() and l2.cpu().numpy().tobytes() == loss.tobytes()
    assert np.isfinite(loss).all() and diff.any()


def test_cpp_trainer_unidirectional_counts_rejected(tmp_path):
    from tests.test_ctc import run_driver
    r = run_driver("train", "lstm", str(tmp_path / "dump.bin"))
    kv = dict(f.split("=") for f in r.stdout.split() if "=" in f)
    print("ctc_test train lstm:", r.stdout.strip(), flush=True)
    assert int(kv["rejected"]) == int(kv["planted_rejected"]) > 0
    assert int(kv["skipped"]) == int(kv["planted_skipped"]) > 0
    assert np.isfinite(float(kv["last_epoch_loss_per_frame"]))


def test_cpp_device_buffer_and_totals_semantics():
    """DeviceBuffer and DeviceTotals, the pieces every owner of device memory in include/ is built from: growing to a smaller size
    keeps the block, growing reports the capacity, a moved-from buffer is null with capacity 0, an empty Upload and a Download of
    nothing do nothing, an untouched totals block reads as zeros and two reads after one call agree."""
    from tests.test_ctc import run_driver
    r = run_driver("buffers")
    kv = dict(f.split("=") for f in r.stdout.split() if "=" in f)
    print("ctc_test buffers:", r.stdout.strip(), flush=True)
    for key in ("grow_smaller_keeps_pointer", "grow_larger_has_capacity", "moved_from_is_empty", "move_assigned_from_is_empty",
                "empty_upload_download_do_nothing", "round_trip", "untouched_totals_are_zero", "totals_read_twice_agree"):
        assert kv[key] == "1", key


def test_cpp_objects_reused_across_shapes():
    """One Ctc, CtcGreedyDecoder, CtcBeamDecoder and CtcAligner through (T 6, S 2), (T 12, S 3, one stream idle), (T 6, S 2): every
    per-stream output has the bits of a fresh object's, and the totals are the three fresh ones added up."""
    from tests.test_ctc import run_driver
    r = run_driver("reuse")
    kv = dict(f.split("=") for f in r.stdout.split() if "=" in f)
    print("ctc_test reuse:", r.stdout.strip(), flush=True)
    assert kv["same0"] == "1" and kv["same1"] == "1" and kv["same2"] == "1"
    assert kv["fresh_totals_counted"] == "1" and int(kv["utterances"]) == 6 and int(kv["frames"]) == 42
    assert kv["totals"] == "1"
