"""Full-size parity of the default paths in a trained-size regime (tests/regimes.py): saturated gates, c at the +-50 clip, max |r| ~ 3,
derivatives up to ~15 -- where the scale-0.01 tests of tests/test_engine_gpu.py run a nearly linear layer.  At 40/800/512 and
512/800/512, T = 20, five or six chained minibatches with carried state and Updates, on the persistent forward chain (folded
recurrence on two fp16 planes, three bf16 planes, fp32 MFMA, or unfolded), the persistent BPTT launch with tail workgroups, the
interleaved chains at 8 and 16 streams and the fused gradient + Update launch.

Bar, per tensor and minibatch: e_eng = relerr(engine, fp64 oracle), e_32 = relerr(fp32 oracle, fp64 oracle), both over max |fp64| of
the tensor; e_eng <= max(4 e_32, floor), floor 1e-5 (out, forward column groups, state, parameter changes) or 2e-5 (in_diff,
derivative column groups, momentum buffers).  The parameters enter as their change theta_k - theta_0.  parity_margins.json records
each tensor's largest e_eng with its bar and, under "<tensor>.ratio", e_eng / e_32 against the bar's ratio; at out_diff scale 1 also
the range-guard events of the engine's fp16-plane products (bar 0).  A failing bar reports those counters with it."""
import numpy as np
import pytest

from tests import regimes as rg
from tests.margins import bound

pytestmark = pytest.mark.gpu

K = 4.0
FLOOR_FWD, FLOOR_BWD = 1e-5, 2e-5
NEAR_CLIP = 1e-3


def _floor(t, floors):
    return floors[1] if (t == "in_diff" or t.startswith("D") or t.startswith("corr.")) else floors[0]


def _check_clip(k, yc_eng, yc_64):
    """The engine clips c at exactly the (frame, cell) entries where the fp64 oracle does, with the same sign; entries within
    NEAR_CLIP of +-50 on either side may go either way."""
    ce, c64 = np.abs(yc_eng), np.abs(yc_64)
    near = (np.abs(ce - rg.CLIP) <= NEAR_CLIP) | (np.abs(c64 - rg.CLIP) <= NEAR_CLIP)
    on_e, on_64 = ce == rg.CLIP, c64 == rg.CLIP
    bad = (on_e != on_64) & ~near
    assert not bad.any(), f"minibatch {k}: clip disagrees at {int(bad.sum())} entries, e.g. {np.argwhere(bad)[:4].tolist()}"
    both = on_e & on_64
    assert np.array_equal(yc_eng[both], yc_64[both]), f"minibatch {k}: clipped with the wrong sign"
    return int(on_e.sum())


def _run(key, flags=0, opts=None, fold_mode=2, persistent=True, floors=(FLOOR_FWD, FLOOR_BWD)):
    """persistent: the persistent launches are expected in minibatches of T >= 8 (the auto policy's threshold); False: never (the
    unfolded chain runs launch per step)."""
    import kaldi_lstm_amd as k
    a = rg.shape_args(key)
    I, C, R, S = a["I"], a["C"], a["R"], a["S"]
    e = k.Engine(I, C, R, S)
    for name, val in (opts or {}).items():
        e.set_option(name, val)
    seen = []

    def on_step(step, eng):
        q = {n: eng.profile_query(n)[1] for n in ("persist_launches", "persist_tail_wgs", "persist_giveups", "fold_mode",
                                                   "fp16_redo_own", "fp16_redo_fold", "fp16_redo_nt", "fp16_redo_outer",
                                                   "fp16_redo_skinny", "tail_merge_timeouts")}
        seen.append(q)

    try:
        recs = rg.run_vs_fp64(e, flags=flags, on_step=on_step, **a)
    finally:
        e.close()

    # the intended path ran, every minibatch
    prev = 0
    for step, q in enumerate(seen):
        if persistent and a["Ts"][step] >= 8:
            assert q["persist_launches"] > prev, f"minibatch {step}: no persistent launch"
            assert q["persist_tail_wgs"] > 0, f"minibatch {step}: no tail workgroups"
        else:
            assert q["persist_launches"] == prev, f"minibatch {step}: a persistent launch where none was expected"
        prev = q["persist_launches"]
        assert q["persist_giveups"] == 0, f"minibatch {step}: a persistent launch gave up"
        assert q["fold_mode"] == fold_mode, f"minibatch {step}: fold_mode {q['fold_mode']} != {fold_mode}"
        if a["od_scale"] == 1.0:
            # nothing here is near the fp16 planes' range: an event would be a spurious guard (and a silent move to the slow path)
            bound(float(q["fp16_redo_own"]), 0.0, "fp16_redo_own")

    # the bar against fp64, with the fp32 oracle's own error as the yardstick
    # (a failure names the range-guard counters: a 16-bit product that consumed an operand >= 16 with no event is a bug)
    clipped = []
    for step, rec in enumerate(recs):
        redo = {n: v for n, v in seen[step].items() if n.startswith("fp16_redo")}
        for t, v in rec.items():
            e32 = rg.relerr(v["f32"], v["f64"])
            een = rg.relerr(v["eng"], v["f64"])
            bar = max(K * e32, _floor(t, floors))
            d32 = max(e32, 1e-30)
            try:
                bound(een / d32, bar / d32, f"{t}.ratio")
                bound(een, bar, t)
            except AssertionError as err:
                raise AssertionError(f"minibatch {step}: {err}; range-guard events so far {redo}") from None
        clipped.append(_check_clip(step, rec["YC"]["eng"], rec["YC"]["f64"]))
    assert all(n > 0 for n in clipped[-2:]), f"the cell clip did not fire: {clipped}"
    return recs, seen


# The fold product on three bf16 planes (six products accumulated into one fp32 sum per k) measures 2-3x the error of the default two
# fp16 planes and of the fp32 MFMA fold at this size (out 6.8e-6 vs 2.1e-6, DC 2.8e-5 vs 6.9e-6, the W_gifo_r momentum buffer 4.7x the
# fp32 oracle's error): its floors are the 50-chunk drift bars (4e-5 / 5e-5) instead of 1e-5 / 2e-5.
_BF16X3_FLOORS = (4e-5, 5e-5)


@pytest.mark.parametrize("flags,opts,fold_mode,persistent,floors", [
    (0, None, 2, True, None),                       # the default: folded recurrence W_rm = W_gifo_r W_r_m on two fp16 planes
    (2, None, 2, True, None),                       # KLSTM_BPTT_FUSE_UPDATE: the gradient products inside klstm_update's launch
    (0, {"fold_bf16x3": 1}, 1, True, _BF16X3_FLOORS),   # three bf16 planes
    (0, {"fold_bf16x3": 0}, 0, True, None),         # fp32 MFMA fold
    (0, {"fold": 0}, 2, False, None),               # the reference-shaped, unfolded chain (launch per step: no persistent launch)
], ids=["plain", "fused", "fold_bf16x3", "fold_f32", "unfolded"])
def test_trained_regime_40_800_512_s4(flags, opts, fold_mode, persistent, floors):
    _run("i40_s4", flags, opts, fold_mode, persistent, floors or (FLOOR_FWD, FLOOR_BWD))


@pytest.mark.parametrize("flags", [0, 2], ids=["plain", "fused"])
@pytest.mark.parametrize("key", ["i40_s8", "i40_s16"])
def test_trained_regime_interleaved_chains(key, flags):
    _run(key, flags)


@pytest.mark.parametrize("key", ["i512_s4", "i512_s4_od2"])
def test_trained_regime_inner_layer(key):
    """configs[3]'s inner layer (x projection outside the chain, two column parts per slot), at out_diff scale 1 and at scale 2, where
    max |dgifo| crosses 16 -- the range guard of the fp16-plane products (2^12-scaled derivative operands) must keep parity there."""
    recs, seen = _run(key)
    if rg.SHAPES[key].get("od_scale", 1.0) > 1.0:
        assert max(rg.max_dgifo(r) for r in recs) >= 16.0, "the case no longer crosses the range guard's 16"


def test_trained_regime_varying_T_and_reset():
    """T = 20, 14, 7, 20, 20, 20: across the fold auto policy's T >= 12 and back (planes re-packed on demand; T = 7 runs launch per
    step), then a reset of the two streams whose c sits at +-50 before the last minibatch."""
    _run("i40_s4_tseq")
