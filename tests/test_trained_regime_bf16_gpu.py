"""The bf16 operand mode (option "bf16") in the trained-size regime of tests/regimes.py: saturated gates, c at the +-50 clip, max |dgifo|
~ 10-22 entering bf16 products -- where the other bf16 parity tests run a nearly linear layer at parameter scale 0.02-0.03.  The paths
are those of BASELINE configs[4] (3 x 1024/512, 32 streams): one forward and one BPTT chain per XCD (klstm_persist_xl.hip), the batched
products of klstm_gemm16.hip (x term, P, d_r + in_diff from the bf16 copies), the bf16 gradient tiles with the fused momentum + Update
epilogue writing those copies; and the launch-per-step bf16 chain a give-up falls back to.

Yardstick (run_bf16_vs_fp64): before every minibatch the engine's parameters theta_k, momentum buffers and carried (c, r) are loaded
into two fp64 oracles, A on theta_k and B on theta_k with W_gifo_x, W_gifo_r and W_r_m rounded to bf16 (RNE); all three sides run the
same minibatch.  E_w = relerr(B, A) is what rounding ONE operand of every weight product to bf16 does to that minibatch; the engine
rounds the OTHER operand (the staged activations / derivatives) with the same unit roundoff and accumulates in fp32, so
E_e = relerr(engine, B) <= 3 E_w per tensor and minibatch (the rule of test_bf16_mode_against_an_error_budget_the_build_did_not_choose;
6 E_w for the peephole gradients, see K_PEEPHOLE_GRAD), with E_w >= 1e-4.  Chained instead of re-anchored, the bf16 perturbation is
chaotic in this regime (B drifts from A to 0.1-0.5 in five minibatches) and a ratio bar would pass anything.  Every column group of both activation slabs is compared (G I F O C H M R,
DG DI DF DO DC DR: each path here materialises all of them), with out, in_diff, the carried state, the momentum buffers and the
parameter change of the minibatch.  The engine also clips c at B's (frame, cell) entries with B's sign, except within
delta = max |YC_B - YC_A| of +-50, and its clip fires in the last two minibatches.  Each ratio E_e / E_w is recorded with the margins
(profiles/trained_regime_bf16_parity_margins.json)."""
import numpy as np
import pytest

from tests import regimes as rg
from tests.margins import bound

pytestmark = pytest.mark.gpu

K = 3.0
# The peephole gradients of a cell that sits at the clip are 50 * (a sum over frames and streams of d_i / d_f / d_o) that cancels
# (40/800/512 x 32, minibatch 4: one cell clipped in 614 of 640 rows, |sum d_o| ~ 1/60 of sum |d_o|).  The engine rounds its
# operands afresh every frame -- errors that add independently through that sum -- while B's rounded weights are one fixed
# perturbation whose effect on it happens to cancel too: measured E_e / E_w up to 4.6 there, 2.02 at most elsewhere.
K_PEEPHOLE_GRAD = 6.0
KERNELS = ("k_fwd_persist_xl", "k_fwd_persist_ms", "k_bwd_persist_xl", "k_gates_step")
COUNTERS = ("persist_giveups", "gemm_copies_launches")


def _check_clip(k, yc_eng, yc_b, yc_a):
    """The engine clips c at exactly B's (frame, cell) entries, with the same sign; entries within delta = max |YC_B - YC_A| (one
    minibatch's bf16 effect on c) of +-50 on either side may go either way."""
    delta = float(np.abs(yc_b - yc_a).max())
    ce, cb = np.abs(yc_eng), np.abs(yc_b)
    near = (np.abs(ce - rg.CLIP) <= delta) | (np.abs(cb - rg.CLIP) <= delta)
    on_e, on_b = ce == rg.CLIP, cb == rg.CLIP
    bad = (on_e != on_b) & ~near
    assert not bad.any(), f"minibatch {k}: clip disagrees at {int(bad.sum())} entries, e.g. {np.argwhere(bad)[:4].tolist()}"
    both = on_e & on_b
    assert np.array_equal(yc_eng[both], yc_b[both]), f"minibatch {k}: clipped with the wrong sign"
    return int(on_e.sum())


def _persistent(a, T):
    """The per-XCD chains take the layer (tests/test_engine_gpu.py _per_xcd_chains) -- in "bf16" = 1 mode, from 9 streams on."""
    C, R, S = a["C"], a["R"], a["S"]
    return C % 32 == 0 and 512 <= C <= 1024 and 9 <= S <= 32 and R % 32 == 0 and 32 <= R <= 512 and T >= 3 and T * S >= 256


def _run(key, flags=0, opts=None, chains=True):
    """chains: the per-XCD chains are expected in every minibatch whose T S reaches 256; False: never (launch per step)."""
    import kaldi_lstm_amd as k
    a = rg.bf16_shape_args(key)
    I, C, R, S = a["I"], a["C"], a["R"], a["S"]
    e = k.Engine(I, C, R, S)
    e.set_option("profile", 1)
    for name, val in dict({"bf16": 1}, **(opts or {})).items():
        e.set_option(name, val)
    seen = []

    def on_step(step, eng):
        seen.append({n: eng.profile_query(n)[1] for n in KERNELS + COUNTERS})

    try:
        recs = rg.run_bf16_vs_fp64(e, flags=flags, on_step=on_step, **a)
    finally:
        e.close()

    # the intended path ran, every minibatch
    prev = dict.fromkeys(KERNELS + COUNTERS, 0)
    xl_before = False
    for step, q in enumerate(seen):
        d = {n: q[n] - prev[n] for n in q}
        xl = chains and _persistent(a, a["Ts"][step])
        assert d["k_fwd_persist_xl"] == (1 if xl else 0), f"minibatch {step}: k_fwd_persist_xl x {d['k_fwd_persist_xl']} ({xl})"
        assert d["k_bwd_persist_xl"] == (1 if xl else 0), f"minibatch {step}: k_bwd_persist_xl x {d['k_bwd_persist_xl']} ({xl})"
        assert d["k_fwd_persist_ms"] == 0, f"minibatch {step}: the one-copy many-stream launch ran"
        if xl:
            assert d["k_gates_step"] == 0, f"minibatch {step}: a step kernel ran next to the chains"
        else:
            assert d["k_gates_step"] > 0, f"minibatch {step}: no launch-per-step chain"
        assert q["persist_giveups"] == 0, f"minibatch {step}: a persistent launch gave up"
        if xl and xl_before:          # d_r + in_diff read the bf16 copies the chain and the previous minibatch's Update wrote
            assert d["gemm_copies_launches"] > 0, f"minibatch {step}: d_r / in_diff not on the bf16 copies"
        elif not xl:
            assert d["gemm_copies_launches"] == 0, f"minibatch {step}: copies form without the per-XCD BPTT chain"
        prev, xl_before = q, xl

    clipped = []
    for step, rec in enumerate(recs):
        for t, v in rec.items():
            if t == "_resets":
                continue
            e_w = rg.relerr(v["B"], v["A"])
            e_e = rg.relerr(v["eng"], v["B"])
            assert e_w >= 1e-4, f"minibatch {step}: {t}: the yardstick is trivial (E_w {e_w:.3g})"
            try:
                bound(e_e / e_w, K_PEEPHOLE_GRAD if t.split(".")[-1].startswith("peephole_") else K, f"{t}.ratio")
            except AssertionError as err:
                raise AssertionError(f"minibatch {step}: {err} (E_e {e_e:.3g}, E_w {e_w:.3g})") from None
        clipped.append(_check_clip(step, rec["YC"]["eng"], rec["YC"]["B"], rec["YC"]["A"]))
    assert all(n > 0 for n in clipped[-2:]), f"the cell clip did not fire: {clipped}"
    return recs, seen


@pytest.mark.parametrize("flags", [0, 2], ids=["plain", "fused"])
def test_bf16_trained_regime_configs4_inner_layer(flags):
    """512/1024/512 x 32: per-XCD chains both ways, bf16 gradient tiles; flags 2 (KLSTM_BPTT_FUSE_UPDATE): the fused momentum + Update
    epilogue writes the bf16 weight copies the next minibatch's d_r / in_diff products read."""
    _run("i512_c1024_s32", flags)


@pytest.mark.parametrize("key", ["i40_c1024_s32", "i512_c1024_s16", "i40_c800_s32", "i512_c800_s32"])
def test_bf16_trained_regime_per_xcd_chains(key):
    """configs[4]'s bottom layer (40 inputs: fp32 batched x term); 16 streams (fewer per XCD group); 800 cells (cell-less slots that
    still project) at 40 and 512 inputs."""
    _run(key)


def test_bf16_trained_regime_launch_per_step_chain():
    """"persist" = 0 at 512/1024/512 x 32: the launch-per-step bf16 chain that a give-up of the per-XCD chains falls back to."""
    _run("i512_c1024_s32", opts={"persist": 0}, chains=False)


def test_bf16_trained_regime_varying_T_and_reset():
    """T = 20, 8, 7, 20, 20, 20 at 32 streams: T S = 256 is the threshold of both per-XCD launches and of the bf16 gradient tiles,
    224 falls back to launch per step; before the last minibatch, half the streams whose c sits at +-50 are reset."""
    recs, _ = _run("i512_c1024_s32_tseq")
    assert 0 < int(recs[-1]["_resets"].sum()) < 32


def test_bf16_trained_regime_forced_bf16_step_kernels():
    """"bf16" = 2 at 40/800/512 x 4: bf16 operands on the launch-per-step kernels below the 9 streams where "bf16" = 1 keeps fp32."""
    _run("i40_c800_s4", opts={"bf16": 2}, chains=False)
