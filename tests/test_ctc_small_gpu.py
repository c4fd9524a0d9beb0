"""klstm_ctc_eval on the device at the smallest shapes at which its indexing can go wrong, against a truth that is exact there
(tests/ctc_ref.py truth64: float64 forward-backward over the RAW posteriors, pinned by enumeration in tests/test_ctc_small.py).

What is enumerated: every label sequence of length 0..3 over the non-blank classes at every length 1..9 frames (ctc_ref.small_grid: all
patterns of equal neighbours, every boundary of the feasibility rule len >= L + repeats, exactly feasible utterances, streams shorter
than the emission look-ahead CTC_DEPTH = 4), under flat, peaked and saturated (exact 0.0 / 1.0) posteriors, for every position of the
blank at K = 2, 3 (scalar path of k_ctc_combine) and 4 (its float4 path).

Forcing a plan.  The chain's geometry follows the label CAPACITY that klstm_ctc_eval derives from the workspace size, not the labels:
launch_ctc (kaldi-lstm_amd/csrc/klstm_ctc.hip) takes N = 2 * capacity + 1 and dispatches
    plan = N <= 64 ? <1,1> : N <= 256 ? <4,1> : N <= 512 ? <4,2> : N <= 1024 ? <16,1> : <16,2>          (<waves, states per thread>)
ctc_eval sizes the workspace from the `longest` of the tuple pack_labels() returned, so passing a larger `longest` with the same tiny
labels selects any plan.  CAPACITIES are both edges of every plan: N = 63, 65, 255, 257, 511, 513, 1023, 1025, 2047 (the upper edge is
exact: one label more needs a wider row, hence a larger workspace).

Bars, per (K, blank, kind) group, pooled over that group's feasible streams; the yardstick is norm_twin, the kernel's RECIPE in numpy
float32 with accurate exp / log, on the same inputs -- never the kernel:
  diff      max |gpu - truth64| <= 4 x max |norm_twin - truth64|
  utt_loss  the same rule on |. - truth64| / max(1, |truth64|)
The factor 4 is room for the chain's fast __expf / __logf and the combine's tree order (expected: about 2).
Conditions, exact, on every call: padding rows and all rows of idle and infeasible streams are 0.0, utt_loss is +inf for an infeasible
stream and 0 for an idle one, the posteriors are unmodified (gpu_eval), totals = (the doubles of the returned losses added in stream
order, utterances, rejected utterances, frames) as the grid gives them."""
import functools

import numpy as np
import pytest
import torch

import kaldi_lstm_amd as k
from tests import ctc_ref as R
from tests.margins import bound
from tests.test_ctc_gpu import gpu_eval

pytestmark = pytest.mark.gpu

CAPACITIES = [31, 32, 127, 128, 255, 256, 511, 512, 1023]
FACTOR = 4.0


def eval_at(c, blank, capacity, totals=None):
    """one call of a small group on the device with the label capacity forced -> (utt_loss [S], diff [T, S, K]) numpy"""
    lab, off, longest = k.ctc.pack_labels(c["labels"], "cuda")
    assert longest <= capacity
    return gpu_eval(c["y"], c["lens"], (lab, off, capacity), blank, totals=totals)


def check_conditions(c, loss, diff, totals=None):
    ok = []
    for s, n in enumerate(c["lens"]):
        assert not diff[n:, s].any(), f"stream {s}: padding rows are not exactly zero"
        if n == 0:
            assert loss[s] == 0.0
        elif c["bad"][s]:
            assert np.isposinf(loss[s]) and not diff[:, s].any(), f"stream {s} {c['lens'][s], c['labels'][s]} is infeasible: loss {loss[s]}"
        else:
            assert np.isfinite(loss[s]), f"stream {s} {c['lens'][s], c['labels'][s]} is feasible: loss {loss[s]}"
            ok.append(s)
    if totals is not None:
        tot = totals.cpu().numpy()
        assert tot[1] == len(ok) and tot[2] == sum(c["bad"]) and tot[3] == sum(c["lens"][s] for s in ok)
        want = 0.0
        for s in ok:                                                   # doubles of floats, added in stream order
            want += float(loss[s])
        assert tot[0] == want
    return ok


def check_bars(e_gpu, r_gpu, e_tw, r_tw, tag):
    print(f"ctc small {tag}: diff gpu {e_gpu:.3g} twin {e_tw:.3g} ratio {e_gpu / e_tw:.3g} | loss gpu {r_gpu:.3g} twin {r_tw:.3g} "
          f"ratio {r_gpu / r_tw:.3g}", flush=True)
    bound(e_gpu, FACTOR * e_tw, "diff vs truth64 (bar: 4 x twin)")
    bound(r_gpu, FACTOR * r_tw, "utt_loss vs truth64, relative to max(1, |truth|) (bar: 4 x twin)")
    bound(e_gpu / e_tw, FACTOR, "diff: gpu / twin")
    bound(r_gpu / r_tw, FACTOR, "utt_loss: gpu / twin")


@pytest.mark.parametrize("kind", R.SMALL_KINDS)
@pytest.mark.parametrize("K,blank", R.SMALL_GROUPS)
def test_small_lattices(K, blank, kind):
    """the whole grid of a group at capacity 31: the single-wave plan <1,1>"""
    e_gpu = r_gpu = e_tw = r_tw = 0.0
    for c in R.small_group(K, blank, kind):
        totals = torch.zeros(4, dtype=torch.float64, device="cuda")
        loss, diff = eval_at(c, blank, 31, totals)
        check_conditions(c, loss, diff, totals)
        e, r = R.pooled_errors(loss, diff, c["l64"], c["d64"], c["lens"], c["bad"])
        e_gpu, r_gpu = max(e_gpu, e), max(r_gpu, r)
        e, r = R.pooled_errors(c["ltw"], c["dtw"], c["l64"], c["d64"], c["lens"], c["bad"])
        e_tw, r_tw = max(e_tw, e), max(r_tw, r)
    check_bars(e_gpu, r_gpu, e_tw, r_tw, f"K={K} blank={blank} {kind}")


@pytest.mark.parametrize("kind", R.SMALL_KINDS)
def test_capacity_changes_no_bit(kind):
    """One 32-stream call at K = 4 under all nine capacities, i.e. all five plans at both of their edges: utt_loss and diff carry the
    bytes of the capacity-31 result.  A state's arithmetic does not depend on the thread that holds it, the row maximum is exact under
    any tree, the emission chain has no multiply to contract, and k_ctc_combine is one kernel -- so a caller who enlarges the workspace
    gets the same gradients."""
    c = R.small_group(4, 0, kind)[0]
    assert len(c["lens"]) == 32
    first = None
    for cap in CAPACITIES:
        totals = torch.zeros(4, dtype=torch.float64, device="cuda")
        loss, diff = eval_at(c, 0, cap, totals)
        check_conditions(c, loss, diff, totals)
        if first is None:
            first = (loss.tobytes(), diff.tobytes())
            continue
        assert loss.tobytes() == first[0], f"{kind}: utt_loss at capacity {cap} differs from capacity 31"
        assert diff.tobytes() == first[1], f"{kind}: diff at capacity {cap} differs from capacity 31"


@functools.lru_cache(maxsize=None)
def edge_case(L):
    """K = 8, blank 0, posteriors softmax(2 randn), five streams around a plan's edge (capacity L: 2L + 1 states on stream 1):
      0  alternating labels, len = L + 2
      1  L equal labels, len = 2L + 1 (two frames to spare): one thread of k_ctc_combine walks a repeat chain of L links
      2  random labels, len = L + repeats: exactly feasible
      3  the same labels, len = 2L + 5
      4  L - 1 alternating labels, len = L - 1: exactly feasible"""
    g = torch.Generator().manual_seed(100 + L)
    K, T = 8, 2 * L + 5
    rnd = (torch.randint(0, K - 1, (L,), generator=g) + 1).tolist()
    rep = sum(a == b for a, b in zip(rnd[:-1], rnd[1:]))
    assert rep > 0
    labels = [[1 + j % 2 for j in range(L)], [3] * L, rnd, rnd, [5 + j % 2 for j in range(L - 1)]]
    lens = [L + 2, 2 * L + 1, L + rep, 2 * L + 5, L - 1]
    y = torch.softmax(2.0 * torch.randn(T, 5, K, generator=g), -1)
    bad = R.infeasible(lens, labels, K, 0, T)
    assert not any(bad)
    l64, d64 = R.truth64(y, lens, labels, 0)
    ltw, dtw = R.twin_batch(y, lens, labels, 0, bad)
    return dict(y=y, lens=lens, labels=labels, bad=bad, l64=l64, d64=d64, ltw=ltw, dtw=dtw)


@pytest.mark.parametrize("L", [31, 32, 127, 128, 255, 256, 511, 512])
def test_plan_edges_with_real_labels(L):
    """every plan with its last (or, one label on, its first) state, slot and wave really in use, under the 4 x twin bars; the exactly
    feasible streams' gamma is one-hot on every frame"""
    c = edge_case(L)
    totals = torch.zeros(4, dtype=torch.float64, device="cuda")
    loss, diff = eval_at(c, 0, L, totals)
    assert check_conditions(c, loss, diff, totals) == [0, 1, 2, 3, 4]
    for s in (2, 4):
        n = c["lens"][s]
        hot = np.zeros((n, 8), np.float32)
        hot[np.arange(n), R.single_path(c["labels"][s], 0)] = 1.0
        err = float(np.abs(diff[:n, s].astype(np.float64) - (c["y"][:n, s].numpy().astype(np.float64) - hot)).max())
        bound(err, 2.0 ** -23, f"stream {s} (exactly feasible): diff - (y - onehot)")
    e_gpu, r_gpu = R.pooled_errors(loss, diff, c["l64"], c["d64"], c["lens"], c["bad"])
    e_tw, r_tw = R.pooled_errors(c["ltw"], c["dtw"], c["l64"], c["d64"], c["lens"], c["bad"])
    check_bars(e_gpu, r_gpu, e_tw, r_tw, f"plan edge L={L}")


def test_mbr_chain_matches_the_loss_on_small_lattices():
    """klstm_ctc_mbr_eval instantiates the same ctc_chain_run: with the list of every stream the single entry "its own labels" (errors
    0), hyp_logp is -utt_loss of klstm_ctc_eval bit for bit under every plan; infeasible entries are -inf with risk -1, idle streams
    risk 0"""
    c = R.small_group(3, 0, "flat")[3]                               # three labels on every stream: the call with repeats and rejections
    S, T = len(c["lens"]), R.SMALL_T
    hyp = np.zeros((S, 1, 3), np.int32)
    hyp_len = np.zeros((S, 1), np.int32)
    for s, lab in enumerate(c["labels"]):
        hyp[s, 0, :len(lab)] = lab
        hyp_len[s, 0] = len(lab)
    arrays = tuple(torch.from_numpy(a).cuda() for a in (hyp, hyp_len, np.ones(S, np.int32), np.zeros((S, 1), np.int32)))
    yd = c["y"].reshape(T * S, 3).cuda().contiguous()
    feasible = [s for s in range(S) if c["lens"][s] > 0 and not c["bad"][s]]
    rejected = [s for s in range(S) if c["bad"][s]]
    idle = c["lens"].index(0)
    assert S == 32 and len(feasible) >= 20 and len(rejected) >= 8
    for cap in (31, 127, 255, 511, 1023):
        loss, diff = eval_at(c, 0, cap)
        check_conditions(c, loss, diff)
        r = k.ctc_mbr_eval(yd, c["lens"], arrays, blank=0, max_len=cap)
        torch.cuda.synchronize()
        logp, risk = r.hyp_logp.cpu().numpy()[:, 0], r.risk.cpu().numpy()
        assert logp[feasible].tobytes() == (-loss[feasible]).tobytes(), f"max_len {cap}: hyp_logp is not -utt_loss of klstm_ctc_eval"
        assert np.isneginf(logp[rejected]).all() and (risk[rejected] == -1.0).all()
        assert (risk[feasible] == 0.0).all() and risk[idle] == 0.0 and np.isneginf(logp[idle])
        assert not r.diff.cpu().numpy().any()                        # one entry, no CTC term: the gradient is exactly zero
