"""The bf16 joint of band-pruned training on the GPU (krnnt_band_eval_bf16 through rnnt_band_eval(precision="bf16")) against
tests/rnnt_band_bf16_ref.py, over the table of tests/test_rnnt_band_gpu.py (J = 16 is a half-full k-panel of 32, J = 48 one and a half).

Parity: max|gpu - truth64| / max|truth64| per tensor against the UNROUNDED float64 reference.  The bar is 2 e_q, e_q the same measure for
the bf16 yardstick evaluated in float64: the quantisation error of the definition, taken from the reference alone.  The kernel commits
the same three roundings (about 1 e_q); the factor 2 is room for f32 accumulation, the hardware tanh (<= 3e-7) and the few elements that
fall on the other side of a rounding boundary, while an indexing, masking or missing-panel error is of relative size 1, hundreds of
e_q.  Where e_q is 0 (the loss at V = 2 or T = 1) the f32 bar of tests/test_rnnt_gpu.py stands in.  The measured fractions are in
profiles/rnnt_band_bf16_margins.json and DESIGN.md 4zc."""
import functools

import numpy as np
import pytest
import torch

from tests import rnnt_band_bf16_ref, rnnt_band_ref, rnnt_ref
from tests.margins import bound
from tests.test_rnnt_band_gpu import CASES, problem, run
from tests.test_rnnt_gpu import FLOOR, MARGIN, SENTINEL, TENSORS, bits, padding_intact, placed

pytestmark = pytest.mark.gpu
f32 = np.float32
RAGGED = (17, 8, 17, 48, 3, 4, "frames", None, 0)


@functools.lru_cache(maxsize=None)
def quantised(case):
    enc, pred, W, b, lens, labels, blank, band = problem(*case)[:8]
    return rnnt_band_bf16_ref.transducer(enc, pred, W, b, lens, labels, blank, band, case[5], torch.float64)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "T%d-U%d-V%d-J%d-S%d-R%d-%s-l%s-b%d" % c)
def test_bf16_eval_against_float64(case):
    T, Umax, V, J, S, R = case[:6]
    enc, pred, W, b, lens, labels, blank, band, truth, twin = problem(*case)
    (ev, eb), (pv, pb) = placed(enc, 0), placed(pred, 1)
    out = {"d_enc": placed(np.full_like(enc, SENTINEL), 1), "d_pred": placed(np.full_like(pred, SENTINEL), 0)}
    totals = torch.zeros(5, dtype=torch.float64, device="cuda")
    res = run(ev, pv, W, b, lens, labels, blank, band, R, totals=totals, out={k: v[0] for k, v in out.items()}, precision="bf16")
    torch.cuda.synchronize()
    assert padding_intact(*out["d_enc"], 1) and padding_intact(*out["d_pred"], 0), "columns outside the rows were written"
    figures = []
    for name in TENSORS:
        err, eq = rnnt_ref.rel_err(res[name].cpu().numpy(), truth[name]), rnnt_ref.rel_err(quantised(case)[name], truth[name])
        bar = 2.0 * eq if eq > 0 else max(MARGIN * rnnt_ref.rel_err(twin[name], truth[name]), FLOOR)
        figures.append((err, bar, name))
        print(f"{case} {name}: {err:.3g} (e_q {eq:.3g}, bar {bar:.3g}, fraction {err / bar:.3f})", flush=True)
    for err, bar, name in figures:
        bound(err, bar, name)
    want = [float(res["loss"].double().sum()), sum(lens), sum(len(y) for y in labels), S, 0]        # (the losses themselves: bounded above)
    assert np.allclose(totals.cpu().numpy(), want, rtol=1e-5)
    if S == 3:                                           # rows t >= T_s of d_enc and u > U_s of d_pred are written as zero
        assert not res["d_pred"].reshape(Umax + 1, S, J)[1:, 1].any() and not res["d_enc"].reshape(T, S, J)[T - 1, 2].any()


def test_rounding_is_to_nearest_and_products_are_exact():
    """|enc + pred| >= 11: h is within 1e-7 of +-1 and bf(h) = +-1 exactly under round to nearest (truncation gives 0.996); W and b are
    k / 64, |k| <= 32, exact in bf16.  The logits are then the same in both precisions and the loss of both entries meets the f32 bar."""
    T, Umax, V, J, R = 17, 5, 17, 48, 8
    rng = np.random.RandomState(11)
    enc, pred = rng.choice([-12.0, 12.0], (T, J)).astype(f32), rng.choice([-1.0, 0.0, 1.0], (Umax + 1, J)).astype(f32)
    W, b = (rng.randint(-32, 33, (V, J)) / 64.0).astype(f32), (rng.randint(-32, 33, V) / 64.0).astype(f32)
    y, band = [[int(v) for v in rng.randint(1, V, Umax)]], np.zeros((1, T), np.int32)
    truth, twin = [rnnt_band_ref.transducer(enc, pred, W, b, [T], y, 0, band, R, dt) for dt in (torch.float64, torch.float32)]
    e32 = rnnt_ref.rel_err(twin["loss"], truth["loss"])
    bar = max(MARGIN * e32, FLOOR)
    assert np.isfinite(twin["loss"]).all() and e32 <= bar                      # the twin itself, on the CPU, before anything runs
    for precision in ("bf16", "f32"):
        res = run(enc, pred, W, b, [T], y, 0, band, R, want_grads=False, precision=precision)
        err = rnnt_ref.rel_err(res["loss"].cpu().numpy(), truth["loss"])
        print(f"saturated {precision} loss: {err:.3g} (twin {e32:.3g}, bar {bar:.3g})", flush=True)
        bound(err, bar, "loss " + precision)


def test_bf16_runs_and_stream_company_leave_the_bits_alone():
    T, Umax, V, J, S, R = RAGGED[:6]
    enc, pred, W, b, lens, labels, blank, band = problem(*RAGGED)[:8]
    one, two, fwd = [run(enc, pred, W, b, lens, labels, blank, band, R, want_grads=g, precision="bf16") for g in (True, True, False)]
    for name in TENSORS:
        assert np.array_equal(bits(one[name]), bits(two[name])), f"{name}: two runs differ"
    assert np.array_equal(bits(one["loss"]), bits(fwd["loss"])) and set(fwd) == {"loss"}
    e3, p3 = enc.reshape(T, S, J), pred.reshape(Umax + 1, S, J)
    for s in range(S):
        sub = run(e3[:, [s]].reshape(-1, J), p3[:, [s]].reshape(-1, J), W, b, [lens[s]], [labels[s]], blank, band[[s]], R, precision="bf16")
        assert bits(sub["loss"])[0] == bits(one["loss"])[s]
        assert np.array_equal(bits(sub["d_enc"].view(T, J)), bits(one["d_enc"].view(T, S, J)[:, s])), s
        assert np.array_equal(bits(sub["d_pred"].view(Umax + 1, J)), bits(one["d_pred"].view(Umax + 1, S, J)[:, s])), s


def test_the_f32_path_is_untouched_by_a_bf16_call():
    enc, pred, W, b, lens, labels, blank, band = problem(*RAGGED)[:8]
    before = run(enc, pred, W, b, lens, labels, blank, band, RAGGED[5])
    half = run(enc, pred, W, b, lens, labels, blank, band, RAGGED[5], precision="bf16")
    after = run(enc, pred, W, b, lens, labels, blank, band, RAGGED[5])
    for name in TENSORS:
        assert np.array_equal(bits(before[name]), bits(after[name])), name
    assert not np.array_equal(bits(half["W_grad"]), bits(before["W_grad"]))    # and the bf16 call was a different computation
