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
