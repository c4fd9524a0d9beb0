"""The trained-size regime of tests/regimes.py, pinned on the two CPU oracles alone (no GPU): the GPU parity tests of that regime
(tests/test_trained_regime_gpu.py) are only informative while the regime stays saturated AND well-conditioned.  If a change to the
recipe makes the network chaotic, the ratio bar against fp64 lets anything pass; if it makes it linear again, the GPU tests see no
more than the scale-0.01 tests do.  Every shape of the GPU cases is checked here."""
import numpy as np
import pytest

from tests import regimes as rg


@pytest.mark.parametrize("key", list(rg.SHAPES))
def test_regime_is_saturated_and_well_conditioned(key):
    a = rg.shape_args(key)
    I, C, R = a["I"], a["C"], a["R"]
    recs = rg.run_vs_fp64(None, **a)
    p0 = rg.trained_params(I, C, R, a["seed"] + 1)
    theta0 = {n: float(np.abs(v).max()) for n, v in rg.split_blob(p0, I, C, R).items()}
    for k, rec in enumerate(recs):
        # not chaotic: the fp32 oracle tracks the fp64 one.  Delta theta is read from fp32 parameters, which store theta_0 + delta to
        # half an ulp of theta_0 per Update: that rounding (not a divergence) is allowed on top.
        for t, v in rec.items():
            err = np.abs(v["f32"] - v["f64"]).max()
            bar = 2e-4 * np.abs(v["f64"]).max()
            if t.startswith("dparams."):
                bar += (k + 1) * 0.5 * np.spacing(np.float32(theta0[t.split(".", 1)[1]]))
            assert err <= bar, f"minibatch {k}: {t}: fp32 vs fp64 {err:.3g} > {bar:.3g}"
        assert rg.saturated_fraction(rec) >= 0.20, f"minibatch {k}: gates not saturated"
        dg = rg.max_dgifo(rec)
        if a["od_scale"] == 1.0:
            assert 4.0 <= dg < 16.0, f"minibatch {k}: max |dgifo| {dg:.3g} outside [4, 16)"
    if a["od_scale"] > 1.0:            # the case that is there to cross the 16 of the fp16-plane products' range guard
        assert max(rg.max_dgifo(r) for r in recs) >= 16.0
    for rec in recs[-2:]:
        assert rg.clipped_count(rec["YC"]["f64"]) >= 10, "the cell clip does not fire"
    assert rg.w_rm_max(I, C, R, p0) >= 0.3


# ---- the bf16 operand mode's shapes (tests/test_trained_regime_bf16_gpu.py), re-anchored per minibatch on the fp64 oracle A ----

def test_oracle_started_from_c_and_r_alone_runs_the_same_minibatch():
    """run_bf16_vs_fp64 loads the oracles' carried block from the engine's (c, r) alone (the state row is 7C + R wide): every other
    column of that block must be dead, or the yardstick would start from a different state than the engine.  Bit-exact, after
    two minibatches have filled the block with carried values of every group."""
    from oracle.oracle import Oracle
    I, C, R, S, T = 40, 64, 32, 3, 6
    p = rg.trained_params(I, C, R, 5)
    rng = np.random.RandomState(6)
    ref = Oracle(I, C, R, S, np.float64)
    ref.set_params(p.astype(np.float64))
    for _ in range(2):
        x, od = rg.trained_inputs(I, R, T, S, rng)
        ref.propagate(x); ref.backpropagate(x, od, momentum=0.9); ref.update(1e-3)
    full = ref.get_state()
    assert np.count_nonzero(full[:, :4 * C]) and np.count_nonzero(full[:, 5 * C:7 * C])
    x, od = rg.trained_inputs(I, R, T, S, rng)
    res = []
    for st in (full, rg.state_row(full[:, 4 * C:5 * C], full[:, 7 * C:], C, R, np.float64)):
        o = Oracle(I, C, R, S, np.float64)
        o.set_params(ref.get_params()); o.set_corr(ref.get_corr()); o.set_state(st)
        res.append(rg._oracle_minibatch(o, x, od, T, None, 1e-3, 0.9, True, ref.get_params()))
    for t in res[0]:
        assert np.array_equal(res[0][t], res[1][t]), t


@pytest.mark.parametrize("key", list(rg.BF16_SHAPES))
def test_bf16_regime_is_saturated_and_its_yardstick_is_informative(key):
    """On the oracles alone, A (fp64, fp32 weights) as the anchor of every minibatch: the regime is saturated (>= 20 % of the gates
    within 0.02 of 0 or 1) and clips (>= 10 entries at +-50 in each of the last two minibatches); the yardstick E_w = relerr(B, A)
    of the bf16 bar is a bf16-sized error on every compared tensor, in [1e-4, 0.2] -- never trivial (a 3 E_w bar would then demand
    more than fp32 can give), never chaotic (it would let anything pass); and the fp32 oracle started from the same anchor stays
    within 2e-4 of A (plus the half ulp of theta per Update that fp32 parameters hold dparams to)."""
    a = rg.bf16_shape_args(key)
    I, C, R = a["I"], a["C"], a["R"]
    recs = rg.run_bf16_vs_fp64(None, with_f32=True, **a)
    theta0 = {n: float(np.abs(v).max()) for n, v in rg.split_blob(rg.trained_params(I, C, R, a["seed"] + 1), I, C, R).items()}
    for k, rec in enumerate(recs):
        for t, v in rec.items():
            if t == "_resets":
                continue
            e_w = rg.relerr(v["B"], v["A"])
            assert 1e-4 <= e_w <= 0.2, f"minibatch {k}: {t}: E_w {e_w:.3g} outside [1e-4, 0.2]"
            err = np.abs(v["f32"] - v["A"]).max()
            bar = 2e-4 * np.abs(v["A"]).max()
            if t.startswith("dparams."):
                bar += 0.5 * np.spacing(np.float32(1.001 * theta0[t.split(".", 1)[1]]))
            assert err <= bar, f"minibatch {k}: {t}: fp32 vs fp64 {err:.3g} > {bar:.3g}"
        sat = rg.saturated_fraction({n: {"f64": rec[n]["A"]} for n in ("YI", "YF", "YO")})
        assert sat >= 0.20, f"minibatch {k}: gates not saturated ({sat:.3f})"
    for k, rec in enumerate(recs[-2:]):
        assert rg.clipped_count(rec["YC"]["A"]) >= 10, f"minibatch {len(recs) - 2 + k}: the cell clip does not fire"
    for k, rst in enumerate(a["resets"] or []):
        if rst == "clipped":
            n = int(recs[k]["_resets"].sum())
            assert 0 < n < a["S"], f"minibatch {k}: {n} of {a['S']} streams sit at +-50"
