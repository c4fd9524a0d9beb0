"""klstm_ctc_mbr_eval on the device at the smallest shapes at which its indexing can go wrong, against a truth that is exact there
(tests/ctc_mbr_ref.py truth64: float64 forward-backward over the RAW posteriors, pinned by path enumeration and central differences
in tests/test_ctc_mbr_small.py).

What is enumerated.  The utterances of ctc_ref.small_grid (every label sequence of length 0..3 at every length 1..9 frames) as the
REFERENCES, every stream listing small_list(): all labellings of length 0, 1, 2 -- the empty one first -- and up to three of length 3,
N = 4 / 7 / 16 (the limit of list_n) at K = 2 / 3 / 4, with the edit distances to the reference as costs.  So every call has entries
that are dropped inside counted streams (a stream of 1..3 frames cannot hold [c0, c0]), streams shorter than the chain's emission
look-ahead, references that are rejected (where lam > 0) and an idle stream; posteriors flat, peaked and saturated (exact 0.0 / 1.0:
most entries run through FLT_MIN clamps and l_q differs by hundreds of nats); (risk_scale, ctc_weight) cycles through (1, 0),
(0.5, 0.3), (4, 0), (0.05, 0.3).  Complete lists (every feasible labelling of K = 3, T <= 4 and K = 2, T <= 5) are held against the
enumeration of all frame paths itself.  Capacities 31 .. 1023 are both edges of all five chain plans (launch_ctc_mbr of
kaldi-lstm_amd/csrc/klstm_ctc_mbr.hip takes NS = 2 * capacity + 1 as launch_ctc does).

Bars, pooled over the counted streams of the calls of a group that share (kappa, lam) -- the floor depends on kappa, so the calls are
not pooled across it; the yardstick is twin32, the recipe documented in include/klstm.h in numpy float32 on the same inputs, never
the kernel.  With Wmax the largest live cost of the pool:
  diff      max |gpu - truth64| <= max(4 x twin's, 2^-21 * max(1, kappa * Wmax))
  risk      the same rule on |risk - truth64|, floor 2^-21 * max(1, kappa * Wmax) * Wmax
  hyp_logp  the same rule on the error relative to max(1, |truth|), floor 2^-21
4 is the factor of tests/test_ctc_small_gpu.py (room for __expf / __logf and the tree order), 2^-21 the floor of
tests/test_ctc_mmi_gpu.py (eight float32 roundings of a value <= 1), scaled by kappa * Wmax because |diff| <= kappa * Wmax.
Measured: profiles/ctc_mbr_small_parity_margins.json."""
import functools

import numpy as np
import pytest
import torch

import kaldi_lstm_amd as k
from tests import ctc_mbr_ref as M
from tests import ctc_ref as R
from tests.margins import bound
from tests.test_ctc_mbr_gpu import gpu_mbr, list_arrays

pytestmark = pytest.mark.gpu

CAPACITIES = [31, 32, 127, 128, 255, 256, 511, 512, 1023]
FACTOR = 4.0
FLOOR = 2.0 ** -21
KEYS = ("risk", "diff", "logp", "post", "ref_loss")


def run(c, max_len=M.SMALL_MAX_LEN, stride=M.SMALL_STRIDE, window=None, kappa=None, lam=None, t64=None):
    """one call dict (ctc_mbr_ref.small_call) on the device: garbage in the slots beyond count, NaN in every row that must not be read
    (the padding rows of a counted stream, all rows of any other), optionally inside a column window; -> (outputs, totals)"""
    kappa, lam, t64 = c["kappa"] if kappa is None else kappa, c["lam"] if lam is None else lam, t64 or c["t64"]
    y = c["y"].clone()
    for s, n in enumerate(c["lens"]):
        y[n if t64["status"][s] == "counted" else 0:, s] = float("nan")
    arrays = list_arrays(c["lists"], c["costs"], c["counts"], c["N"], stride, garbage=True)
    totals = torch.zeros(6, dtype=torch.float64, device="cuda")
    pad, off = window or (0, 0)
    out = gpu_mbr(y, c["lens"], arrays, c["refs"], c["blank"], kappa, lam, max_len, pad, off, totals)
    return out, totals.cpu().numpy()


def check_exact(c, out, totals, t64, kappa, lam):
    """what holds exactly on every call: statuses and dropped entries as truth64 says, zeros where nothing is counted, the six totals"""
    lens, N, K = c["lens"], c["N"], c["K"]
    status = t64["status"]
    counted = [s for s in range(len(lens)) if status[s] == "counted"]
    assert (out["ref_loss"] is None) == (lam == 0)
    for s, n in enumerate(lens):
        if status[s] != "counted":
            assert not out["diff"][:, s].any(), f"stream {s} ({status[s]}): diff rows are not exactly zero"
            assert out["risk"][s] == (0.0 if status[s] == "idle" else -1.0), (s, status[s], out["risk"][s])
            assert np.isneginf(out["logp"][s]).all() and not out["post"][s].any()
            assert lam == 0 or out["ref_loss"][s] == 0.0
            continue
        assert not out["diff"][n:, s].any(), f"stream {s}: padding rows are not exactly zero"
        live = t64["live"][s]
        dead = [q for q in range(N) if q not in live]
        assert np.isfinite(out["logp"][s, live]).all() and (out["post"][s, live] >= 0).all(), (s, lens[s], c["refs"][s])
        assert np.isneginf(out["logp"][s, dead]).all() and not out["post"][s, dead].any(), f"stream {s}: a dropped entry counts"
        assert np.isfinite(out["diff"][:n, s]).all() and np.isfinite(out["risk"][s])
        bound(abs(float(out["post"][s].astype(np.float64).sum()) - 1.0), 1e-6, "sum_q post - 1")
        if lam == 0:                                                 # the risk part sums to zero over the classes of a row
            wmax = max(c["costs"][s][q] for q in live)
            bound(float(np.abs(out["diff"][:n, s].astype(np.float64).sum(-1)).max()), K * 2.0 ** -23 * (1 + kappa * wmax), "sum_k diff")
        else:
            assert np.isfinite(out["ref_loss"][s])
    assert totals[0] == sum(float(out["risk"][s]) for s in counted) and totals[1] == sum(c["costs"][s][0] for s in counted)
    assert totals[2] == len(counted) and totals[3] == sum(st in ("rejected", "skipped") for st in status)
    assert totals[4] == sum(lens[s] for s in counted)
    assert totals[5] == (sum(float(out["ref_loss"][s]) for s in counted) if lam > 0 else 0.0)


class Bars:
    """the pooled errors of the device and of the twin, per (kappa, lam)"""

    def __init__(self):
        self.pools = {}

    def add(self, c, out, t64, tw, kappa, lam):
        gpu = dict(diff=out["diff"], risk=out["risk"], logp=[out["logp"][s, live] for s, live in enumerate(t64["live"])])
        g, t = M.pooled(gpu, t64, c["lens"], c["costs"]), M.pooled(tw, t64, c["lens"])
        p = self.pools.setdefault((kappa, lam), [0.0] * 7)
        self.pools[(kappa, lam)] = [max(a, b) for a, b in zip(p, g[:3] + t[:3] + (g[3],))]

    def check(self, tag):
        assert self.pools
        for (kappa, lam), (e_g, r_g, l_g, e_t, r_t, l_t, wmax) in sorted(self.pools.items()):
            scale = max(1.0, kappa * wmax)
            print(f"mbr small {tag} kappa={kappa:.3g} lam={lam:.3g} Wmax={wmax}: diff gpu {e_g:.3g} twin {e_t:.3g} | risk gpu {r_g:.3g} twin "
                  f"{r_t:.3g} | logp gpu {l_g:.3g} twin {l_t:.3g}", flush=True)
            assert wmax >= 1 and np.isfinite([e_t, r_t, l_t]).all()
            bound(e_g, max(FACTOR * e_t, FLOOR * scale), "diff vs truth64 (bar: 4 x twin, floor 2^-21 max(1, kappa Wmax))")
            bound(r_g, max(FACTOR * r_t, FLOOR * scale * wmax), "risk vs truth64 (bar: 4 x twin, floor 2^-21 max(1, kappa Wmax) Wmax)")
            bound(l_g, max(FACTOR * l_t, FLOOR), "hyp_logp vs truth64, relative to max(1, |truth|) (bar: 4 x twin, floor 2^-21)")
            # the same three bars as ratios, so that gpu / twin itself is on record
            for what, g, t, floor in (("diff", e_g, e_t, FLOOR * scale), ("risk", r_g, r_t, FLOOR * scale * wmax), ("hyp_logp", l_g, l_t, FLOOR)):
                if t > 0:
                    bound(g / t, max(FACTOR, floor / t), f"{what}: gpu / twin")


def check_relation_with_ctc_eval(c, out, t64, lam):
    """hyp_logp[:, q] of every live entry carries the bytes of -utt_loss of klstm_ctc_eval called with that entry as the label, ref_loss
    those of the reference"""
    T, S, K = c["y"].shape
    yd = c["y"].reshape(T * S, K).cuda().contiguous()
    for q in range(c["N"]):
        streams = [s for s in range(S) if q in t64["live"][s]]
        if not streams:
            continue
        labels = [c["lists"][s][q] if s in streams else [] for s in range(S)]
        loss = k.ctc_eval(yd, c["lens"], labels, blank=c["blank"])[0].cpu().numpy()
        assert np.isfinite(loss[streams]).all()
        assert (-loss[streams]).tobytes() == out["logp"][streams, q].tobytes(), f"entry {q}: hyp_logp is not -utt_loss of klstm_ctc_eval"
    if lam > 0:
        counted = [s for s in range(S) if t64["status"][s] == "counted"]
        loss = k.ctc_eval(yd, c["lens"], c["refs"], blank=c["blank"])[0].cpu().numpy()
        assert loss[counted].tobytes() == out["ref_loss"][counted].tobytes(), "ref_loss is not utt_loss of klstm_ctc_eval"


def window_of(K, blank, call):
    """K = 3 at blank 1 and K = 4 at blank 3: every second call inside a column window (K = 4: in turn rows that stay 16-byte aligned,
    the float4 path with a stride, and an odd offset, the scalar path)"""
    if (K, blank) not in ((3, 1), (4, 3)) or call % 2 == 0:
        return None
    return (5, 1) if K == 3 else ((4, 0) if call % 4 == 1 else (3, 1))


@pytest.mark.parametrize("kind", R.SMALL_KINDS)
@pytest.mark.parametrize("K,blank", R.SMALL_GROUPS)
def test_small_lists(K, blank, kind):
    """every call of a group at max_len 31 and hyp_stride 3: the bars, the exact conditions, and the relation with klstm_ctc_eval"""
    bars = Bars()
    for i, c in enumerate(M.small_group(K, blank, kind)):
        out, totals = run(c, window=window_of(K, blank, i))
        check_exact(c, out, totals, c["t64"], c["kappa"], c["lam"])
        check_relation_with_ctc_eval(c, out, c["t64"], c["lam"])
        bars.add(c, out, c["t64"], c["tw"], c["kappa"], c["lam"])
    bars.check(f"K={K} blank={blank} {kind}")


@pytest.mark.parametrize("kind", R.SMALL_KINDS)
def test_capacity_changes_no_bit(kind):
    """One 32-stream call at K = 4 (16 entries and the reference: E = 17, lam = 0.3) under all nine capacities, i.e. all five chain
    plans at both of their edges: risk, diff, hyp_logp, hyp_post and ref_loss carry the bytes of the max_len = 31 result"""
    c = M.small_group(4, 0, kind)[1]
    assert len(c["lens"]) == 32 and c["N"] == 16 and abs(c["lam"] - 0.3) < 1e-6
    t = c["t64"]
    moving = sum(float(np.abs(t["diff"][:, s]).max()) > 1e-3 for s in range(32))
    assert moving >= 20, f"only {moving} streams with a gradient beyond 1e-3"
    first = None
    for cap in CAPACITIES:
        assert k.ctc_mbr_workspace_bytes(R.SMALL_T, 32, 16, cap, True) < 100 << 20
        out, totals = run(c, max_len=cap)
        check_exact(c, out, totals, t, c["kappa"], c["lam"])
        if first is None:
            first = out
            continue
        for key in KEYS:
            assert out[key].tobytes() == first[key].tobytes(), f"{kind}: {key} at max_len {cap} differs from max_len 31"


@pytest.mark.parametrize("kind", R.SMALL_KINDS)
def test_complete_list_is_the_true_posterior(kind):
    """the complete lists of tests/test_ctc_mbr_small.py (stream s: s + 1 frames, every labelling feasible there; unlisted slots hold
    garbage) at kappa = 1, lam = 0: risk and diff against the sums over all K^T frame paths, and the listed probabilities add up to the
    product of the row sums"""
    for K, blank in [g for g in R.SMALL_GROUPS if g[0] in M.COMPLETE_T]:
        c = M.complete_case(K, blank, kind)
        T = len(c["lens"])
        t64 = dict(c["t64"])
        t64["risk"] = np.array([e["risk"] for e in c["enum"]])
        t64["diff"] = np.zeros_like(c["t64"]["diff"])
        for s, n in enumerate(c["lens"]):
            t64["diff"][:n, s] = c["enum"][s]["diff"]
        t64["logp"] = [list(e["logp"]) for e in c["enum"]]
        out, totals = run(c, stride=T)
        check_exact(c, out, totals, t64, 1.0, 0.0)
        bars = Bars()
        bars.add(c, out, t64, c["tw"], 1.0, 0.0)
        bars.check(f"complete lists K={K} blank={blank} {kind}")
        m_gpu = m_tw = 0.0
        for s, n in enumerate(c["lens"]):
            rows = float(np.prod(c["yd"][:n, s].sum(-1)))
            cnt = c["counts"][s]
            m_gpu = max(m_gpu, abs(float(np.exp(out["logp"][s, :cnt].astype(np.float64)).sum()) - rows) / max(1.0, rows))
            m_tw = max(m_tw, abs(float(np.exp(np.array(c["tw"]["logp"][s])).sum()) - rows) / max(1.0, rows))
        print(f"complete lists K={K} blank={blank} {kind}: sum_q exp(hyp_logp) - prod row sums: gpu {m_gpu:.3g} twin {m_tw:.3g}", flush=True)
        bound(m_gpu, max(FACTOR * m_tw, FLOOR), "sum_q exp(hyp_logp) vs the product of the row sums (bar: 4 x twin, floor 2^-21)")


@functools.lru_cache(maxsize=None)
def edge_case(L):
    """K = 8, blank 0, posteriors softmax(2 randn), T = 2L + 5, three streams of three entries around a plan's edge (max_len = L):
      0  len T: L random labels with at least one repeat; the same with the middle label substituted; the first L - 1 of them
      1  len 2L + 1: L equal labels (one thread of k_mbr_combine walks a chain of L links); L - 1 of them; L - 1 and one other
      2  len L + repeats of its first entry, which is therefore exactly feasible; a variant with one more repeat, infeasible at this
         length and hence dropped; its first L - 1 labels
    costs 0, 1, 2 in some order, lam = 0.3 with the first entry as the reference.  kappa, from the truth's log probabilities alone: the
    power of two at which the runner-up of streams 0 and 1 is exp(-4) of the best or closer, 1 at the most"""
    g = torch.Generator().manual_seed(300 + L)
    K, T = 8, 2 * L + 5
    a = (torch.randint(0, K - 1, (L,), generator=g) + 1).tolist()
    b = (torch.randint(0, K - 1, (L,), generator=g) + 1).tolist()
    rep_a, rep_b = (sum(u == v for u, v in zip(x[:-1], x[1:])) for x in (a, b))
    assert rep_a > 0 and rep_b > 0
    mid = L // 2
    a2 = list(a)
    a2[mid] = next(v for v in range(1, K) if v not in (a[mid - 1], a[mid], a[mid + 1]))
    j = next(j for j in range(1, L) if b[j] != b[j - 1] and (j + 1 == L or b[j + 1] not in (b[j - 1], b[j])))
    b2 = list(b)
    b2[j] = b[j - 1]                                               # one repeat more than b: needs len + 1 frames
    assert sum(u == v for u, v in zip(b2[:-1], b2[1:])) == rep_b + 1
    lists = [[a, a2, a[:-1]], [[3] * L, [3] * (L - 1), [3] * (L - 1) + [5]], [b, b2, b[:-1]]]
    costs = [[0, 1, 2], [1, 0, 2], [2, 1, 0]]
    lens = [T, 2 * L + 1, L + rep_b]
    refs = [l[0] for l in lists]
    y = torch.softmax(2.0 * torch.randn(T, 3, K, generator=g), -1)
    c = dict(y=y, lens=lens, refs=refs, lists=lists, costs=costs, counts=[3, 3, 3], N=3, K=K, blank=0)
    lam = 0.3
    probe = M.truth64(y, lens, lists, costs, c["counts"], refs, 0, 1.0, lam, 3, L, L)
    gap = max(sorted(probe["logp"][s])[-1] - sorted(probe["logp"][s])[-2] for s in (0, 1))
    kappa = min(1.0, 2.0 ** np.floor(np.log2(4.0 / gap)))
    args = (y, lens, lists, costs, c["counts"], refs, 0, kappa, lam, 3, L, L)
    c.update(kappa=float(kappa), lam=float(np.float32(lam)), t64=M.truth64(*args), tw=M.twin32(*args))
    return c


@pytest.mark.parametrize("L", [31, 32, 127, 128, 255, 256, 511, 512])
def test_plan_edges_with_lists(L):
    """every plan with its last (or, one label on, its first) state, slot and wave really in use by several entries whose P is not
    one-hot, under the bars of test_small_lists; the dropped entry sits between two live ones"""
    c = edge_case(L)
    t = c["t64"]
    assert t["status"] == ["counted"] * 3 and t["dropped"] == [[False] * 3, [False] * 3, [False, True, False]]
    second = [sorted(t["post"][s])[-2] for s in (0, 1)]
    print(f"mbr plan edge L={L}: kappa {c['kappa']:.4g}, second-largest P of streams 0 and 1: {second[0]:.3g} {second[1]:.3g}", flush=True)
    assert min(second) >= 1e-3
    assert k.ctc_mbr_workspace_bytes(2 * L + 5, 3, 3, L, True) < 110 << 20
    out, totals = run(c, max_len=L, stride=L)
    check_exact(c, out, totals, t, c["kappa"], c["lam"])
    bars = Bars()
    bars.add(c, out, t, c["tw"], c["kappa"], c["lam"])
    bars.check(f"plan edge L={L}")


@pytest.mark.parametrize("kappa", [1e-3, 50.0])
def test_risk_scale_extremes(kappa):
    """one flat K = 4 call (references of two and three labels, 16 entries) at a risk scale that makes P uniform and at one that makes
    it one-hot: the bars of test_small_lists, every output finite on the counted streams, the rows of the risk part sum to zero"""
    c = M.small_group(4, 0, "flat")[3]
    kappa = float(np.float32(kappa))
    args = (c["y"], c["lens"], c["lists"], c["costs"], c["counts"], c["refs"], 0, kappa, 0.0, 16, M.SMALL_MAX_LEN, M.SMALL_STRIDE)
    t, tw = M.truth64(*args), M.twin32(*args)
    counted = [s for s in range(32) if t["status"][s] == "counted"]
    assert len(counted) == 31
    if kappa < 1:
        worst = max(float(np.abs(np.array(t["post"][s]) - 1.0 / len(t["post"][s])).max()) for s in counted)
        assert worst <= 1e-2, f"P is not uniform within 1e-2: {worst:.3g}"
    else:
        hot = sum(max(t["post"][s]) >= 1.0 - 1e-6 for s in counted)
        assert hot >= 20, f"P is one-hot within 1e-6 on {hot} streams only"
    out, totals = run(c, kappa=kappa, lam=0.0, t64=t)
    check_exact(c, out, totals, t, kappa, 0.0)                       # finite outputs and the row sums are among its conditions
    bars = Bars()
    bars.add(c, out, t, tw, kappa, 0.0)
    bars.check(f"risk scale {kappa:.3g}")
