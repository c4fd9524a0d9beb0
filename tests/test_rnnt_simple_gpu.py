"""The simple-joiner loss and the band it selects on the GPU (krnnt_simple_eval, krnnt_band_from_occupation of include/klstm_rnnt.h)
against tests/rnnt_simple_ref.py, and the C++ layer over them (Transducer::EvalSimple / BandFromOccupation) through
tests/cpp/rnnt_simple_test.cpp.

Parity: the measure and the bar of tests/test_rnnt_gpu.py, imported from there unchanged: max|gpu - truth64| / max|truth64| per tensor
through margins.bound(), bar = max(MARGIN x the error of the float32 twin on the same inputs, FLOOR).  The measured figures are in
profiles/rnnt_simple_margins.json and DESIGN.md 4zb.  The shapes sit at the edges of the tiles of klstm_rnnt_simple.hip (16 frames x 64
label positions per normaliser tile, 16 x 16 per wave, K panels of 32 classes, 16 rows x 128 classes per gradient tile, gradient K
panels of 32 label positions / frames): the table of the issue needed no change.  Logits are drawn with a spread of at most 12."""
import functools

import numpy as np
import pytest
import torch

from tests import cpp_driver, rnnt_simple_ref
from tests.margins import bound
from tests.rnnt_ref import rel_err
from tests.test_rnnt_band_gpu import valid
from tests.test_rnnt_gpu import FLOOR, MARGIN, SENTINEL, bits, padding_intact, placed

pytestmark = pytest.mark.gpu
f32 = np.float32
TENSORS = ("loss", "d_am", "d_lm", "occ")
# (T, Umax, V, S, blank is V - 1)
CASES = [(1, 0, 2, 1, 0), (5, 3, 5, 1, 1), (16, 15, 32, 1, 0), (17, 16, 33, 3, 1), (33, 63, 130, 3, 0), (17, 64, 17, 1, 1), (40, 70, 5, 1, 0)]


@functools.lru_cache(maxsize=None)
def problem(T, Umax, V, S, blank_last, seed=0):
    """inputs (ragged at S = 3: a repeated label at full length, U = 0, T_s < T) and both references"""
    rng = np.random.RandomState(seed + 7 * T + Umax)
    blank = V - 1 if blank_last else 0
    am, lm = rng.uniform(-3, 3, (T * S, V)).astype(f32), rng.uniform(-3, 3, ((Umax + 1) * S, V)).astype(f32)
    lens, ulen = [T] * S, [Umax] * S
    if S == 3:
        lens, ulen = [T, T, max(T - 1, 1)], [Umax, 0, max(Umax - 1, 0)]
    labels = [[int(v) for v in (rng.randint(0, V - 1, n) + (blank == 0))] for n in ulen]
    if Umax >= 2:
        labels[0][1] = labels[0][0]
    refs = [rnnt_simple_ref.simple(am, lm, lens, labels, blank, dt) for dt in (torch.float64, torch.float32)]
    return am, lm, lens, labels, blank, refs[0], refs[1]


def run(am, lm, lens, labels, blank, **kw):
    import kaldi_lstm_amd as k
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=f32)).cuda() if isinstance(x, np.ndarray) else x
    return k.rnnt_simple_eval(d(am), d(lm), lens, labels, blank=blank, **{"want_occ": True, **kw})


def check(tag, res, truth, twin):
    figures = []
    for name in TENSORS:
        err, e32 = rel_err(res[name].cpu().numpy(), truth[name]), rel_err(twin[name], truth[name])
        figures.append((err, max(MARGIN * e32, FLOOR), name))
        print(f"{tag} {name}: {err:.3g} (twin {e32:.3g}, bar {figures[-1][1]:.3g})", flush=True)
    for err, bar, name in figures:
        bound(err, bar, name)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "T%d-U%d-V%d-S%d-b%d" % c)
def test_simple_eval_against_float64(case):
    T, Umax, V, S = case[:4]
    am, lm, lens, labels, blank, truth, twin = problem(*case)
    (av, ab), (lv, lb) = placed(am, 0), placed(lm, 1)
    out = {"d_am": placed(np.full_like(am, SENTINEL), 1), "d_lm": placed(np.full_like(lm, SENTINEL), 0)}
    totals = torch.zeros(5, dtype=torch.float64, device="cuda")
    res = run(av, lv, lens, labels, blank, totals=totals, out={k: v[0] for k, v in out.items()})
    torch.cuda.synchronize()
    assert padding_intact(*out["d_am"], 1) and padding_intact(*out["d_lm"], 0), "columns outside the rows were written"
    assert padding_intact(av, ab, 0) and padding_intact(lv, lb, 1)
    check("%s" % (case,), res, truth, twin)
    assert np.allclose(totals.cpu().numpy(), [truth["loss"].sum(), sum(lens), sum(len(y) for y in labels), S, 0], rtol=1e-5)
    if S == 3:                                           # rows t >= T_s of d_am and u > U_s of d_lm, and occ outside the lattice: zero
        assert not res["d_lm"].reshape(Umax + 1, S, V)[1:, 1].any() and not res["d_am"].reshape(T, S, V)[T - 1, 2].any()
        assert not res["occ"][1, :, 1:].any() and not res["occ"][2, T - 1].any()


def test_long_lattice_keeps_its_digits():
    """T = 400, U = 60, V = 4: log alpha reaches about -400; the same bar holds (the lattice kernels of krnnt_eval run in double)"""
    rng = np.random.RandomState(5)
    T, U, V = 400, 60, 4
    am, lm = rng.uniform(-3, 3, (T, V)).astype(f32), rng.uniform(-3, 3, (U + 1, V)).astype(f32)
    y = [[int(v) for v in rng.randint(1, V, U)]]
    truth, twin = [rnnt_simple_ref.simple(am, lm, [T], y, 0, dt) for dt in (torch.float64, torch.float32)]
    check("long", run(am, lm, [T], y, 0), truth, twin)


def test_runs_and_stream_company_leave_the_bits_alone_and_a_bad_label_is_rejected():
    case = (17, 16, 33, 3, 1)
    T, Umax, V, S = case[:4]
    am, lm, lens, labels, blank = problem(*case)[:5]
    one, two, fwd = [run(am, lm, lens, labels, blank, want_grads=g, want_occ=g) for g in (True, True, False)]
    for name in TENSORS:
        assert np.array_equal(bits(one[name]), bits(two[name])), f"{name}: two runs differ"
    assert np.array_equal(bits(one["loss"]), bits(fwd["loss"])) and set(fwd) == {"loss"}
    a3, l3 = am.reshape(T, S, V), lm.reshape(Umax + 1, S, V)

    def same(sub, order):
        n = len(order)
        for i, s in enumerate(order):
            assert bits(sub["loss"])[i] == bits(one["loss"])[s] and np.array_equal(bits(sub["occ"][i]), bits(one["occ"][s])), (order, s)
            assert np.array_equal(bits(sub["d_am"].view(T, n, V)[:, i]), bits(one["d_am"].view(T, S, V)[:, s])), (order, s)
            assert np.array_equal(bits(sub["d_lm"].view(Umax + 1, n, V)[:, i]), bits(one["d_lm"].view(Umax + 1, S, V)[:, s])), (order, s)

    for order in ([0], [1], [2], [2, 0, 1]):
        same(run(a3[:, order].reshape(-1, V), l3[:, order].reshape(-1, V), [lens[s] for s in order], [labels[s] for s in order], blank), order)
    bad = [list(y) for y in labels]
    bad[2][0] = blank                                    # stream 2 carries the blank as a label: rejected, its rows untouched
    out = {"d_am": torch.full((T * S, V), SENTINEL, device="cuda"), "d_lm": torch.full(((Umax + 1) * S, V), SENTINEL, device="cuda"),
           "occ": torch.full((S, T, Umax + 1), SENTINEL, device="cuda")}
    totals = torch.zeros(5, dtype=torch.float64, device="cuda")
    res = run(am, lm, lens, bad, blank, out=out, totals=totals)
    same({k: (v[:2] if k in ("loss", "occ") else v.view(-1, S, V)[:, :2].reshape(-1, V)) for k, v in res.items()}, [0, 1])
    assert float(res["loss"][2]) == 0.0 and totals.cpu().numpy()[3:].tolist() == [3, 1]
    assert bool((res["d_am"].view(T, S, V)[:, 2] == SENTINEL).all()) and bool((res["d_lm"].view(-1, S, V)[:, 2] == SENTINEL).all())
    assert bool((res["occ"][2] == SENTINEL).all())


@pytest.mark.parametrize("R", [1, 4, 9, 64])
@pytest.mark.parametrize("plane", ["floats", "ties", "ridge"])
def test_band_from_occupation_is_the_rule(R, plane):
    """on GIVEN planes, exactly: streams across the chunk of 256 frames of the scans and the 64 lanes of the arg-max, U = 0, an idle
    stream, and (9, 9 R), which no band of width R can serve (a row of -1); small integers give ties, which go to the lower k.  Pure
    noise jumps too far between frames for a narrow band (the rule answers -1 there as well), so a third plane carries a ridge of mass
    along the straight line under the noise: its bands are valid rows at every R > 1"""
    import kaldi_lstm_amd as k
    rng = np.random.RandomState(R)
    lens, ulen = [600, 257, 40, 0, 9], [70, 300, 0, 0, 9 * R]
    occ = rng.randint(0, 3, (5, 600, max(ulen) + 1)).astype(f32) if plane == "ties" else rng.rand(5, 600, max(ulen) + 1).astype(f32)
    if plane == "ridge":
        for s in (0, 1):
            occ[s, np.arange(lens[s]), np.arange(lens[s]) * ulen[s] // lens[s]] += R + 1
    got = k.rnnt_band_from_occupation(torch.from_numpy(occ).cuda(), lens, [[1] * n for n in ulen], R).cpu().numpy()
    assert got.shape == (5, 600)
    for s, (Ts, U) in enumerate(zip(lens, ulen)):
        want = rnnt_simple_ref.band_rule(occ[s], Ts, U, R)
        assert got[s, :Ts].tolist() == want, s
        assert (got[s, Ts:] == (want[-1] if Ts else 0)).all() and (want[:1] in ([], [-1]) or valid(want, U, R)), s
    assert got[4, 0] == -1 and (plane != "ridge" or R == 1 or (got[0, 0] == 0 and got[1, 0] == 0))


def test_the_band_of_the_simple_pass_holds_a_planted_alignment_and_band_eval_accepts_it():
    """am favours y_i at frame f_i and blank elsewhere by a margin of 6 (an alignment off the planted one loses e^-6 per step, so the
    occupation sits on the path: asserted on the float64 reference first); lm is flat"""
    import kaldi_lstm_amd as k
    rng = np.random.RandomState(11)
    T, V, S, R, J, margin = 48, 9, 3, 4, 16, 6.0
    lens, labels = [48, 40, 48], [[1 + (3 * i + n) % (V - 1) for i in range(n)] for n in (20, 7, 0)]     # no label twice in a row
    Umax = 20
    frames = [sorted(int(f) for f in rng.choice(Ts - 1, len(y), replace=False)) for Ts, y in zip(lens, labels)]
    am, lm = np.zeros((T, S, V), f32), np.zeros(((Umax + 1) * S, V), f32)
    am[:, :, 0] = margin
    for s in range(S):
        for f, y in zip(frames[s], labels[s]):
            am[f, s, 0], am[f, s, y] = 0.0, margin
    am = am.reshape(T * S, V)
    path = [[(t, sum(f < t for f in frames[s])) for t in range(lens[s])] + [(f, i + 1) for i, f in enumerate(frames[s])] for s in range(S)]

    def holds(s, u0):
        return valid(u0, len(labels[s]), R) and all(u0[t] <= u <= u0[t] + R - 1 for t, u in path[s])

    ref = rnnt_simple_ref.simple(am, lm, lens, labels, 0, torch.float64)["occ"].astype(f32)
    assert all(holds(s, rnnt_simple_ref.band_rule(ref[s], lens[s], len(labels[s]), R)) for s in range(S)), "the reference's band misses the path"
    d = lambda x: torch.from_numpy(x).cuda()
    band = k.rnnt_band_from_occupation(k.rnnt_simple_eval(d(am), d(lm), lens, labels, want_grads=False, want_occ=True)["occ"], lens, labels, R)
    assert all(holds(s, band[s, :lens[s]].tolist()) for s in range(S))
    totals = torch.zeros(5, dtype=torch.float64, device="cuda")
    res = k.rnnt_band_eval(d(rng.randn(T * S, J).astype(f32)), d(rng.randn((Umax + 1) * S, J).astype(f32)), d(rng.uniform(-.3, .3, (V, J)).astype(f32)),
                           d(np.zeros(V, f32)), lens, labels, band, R, totals=totals)
    assert totals.cpu().numpy()[3:].tolist() == [3, 0] and bool(torch.isfinite(res["loss"]).all()) and bool((res["loss"] > 0).all())


def test_the_cpp_holder_is_the_python_path():
    """tests/cpp/rnnt_simple_test.cpp: Transducer::EvalSimple + BandFromOccupation on inputs from a 32-bit generator that is repeated here"""
    import kaldi_lstm_amd as k
    T, Umax, V, S, R = 21, 6, 37, 2, 3
    state = [12345]

    def gen(n):
        out = np.empty(n, f32)
        for i in range(n):
            state[0] = (state[0] * 1664525 + 1013904223) & 0xFFFFFFFF
            out[i] = f32(4) * (f32(((state[0] >> 8) & 0xFFFF) / 65536.0) - f32(0.5))
        return torch.from_numpy(out).cuda()

    am, lm = gen(T * S * V).view(T * S, V), gen((Umax + 1) * S * V).view(-1, V)
    lens, labels = [T, T - 4], [[1, 2, 2, 3, 4, 36], [5, 1, 3]]
    res = k.rnnt_simple_eval(am, lm, lens, labels, want_occ=True)
    band = k.rnnt_band_from_occupation(res["occ"], lens, labels, R)
    want = [int(v) for v in bits(res["loss"])] + [int(bits(res[n]).astype(np.uint64).sum()) for n in ("d_am", "d_lm")] + band.flatten().tolist()
    got = cpp_driver.run("rnnt_simple_test").stdout.split()
    assert got[0] == "OK" and [int(v) for v in got[1:]] == want
