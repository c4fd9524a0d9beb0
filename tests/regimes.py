"""A trained-size regime for full-size LSTM parity, and a runner that puts the engine next to the fp32 AND the fp64 oracle.

make_params(scale=0.01) keeps the layer nearly linear (no gate near 0 or 1, max |c| ~ 0.1, the cell clip never fires); uniform
weights at scale >= 0.2 make the random network chaotic (fp32 and fp64 oracles disagree completely within 20-40 frames), so a ratio
bar against fp64 lets anything pass there.  trained_params() builds the regime per tensor instead: the gates saturate (~30 % of
them within 0.02 of 0 or 1), c reaches the +-50 clip, max |r| ~ 3, max |dgifo| ~ 10 at out_diff ~ N(0, 1) -- and fp32 still
tracks fp64 to ~1e-5 over chained minibatches.  tests/test_trained_regime.py pins those properties on the oracles alone.

The truth is the fp64 oracle; the yardstick of an engine's error is the fp32 oracle's own error against fp64 (run_vs_fp64)."""
import numpy as np

from oracle.oracle import Oracle, param_sizes, split_blob

MOMENTUM = 0.9
LR = 2e-5           # moves the parameters by ~1e-3 of their maximum per Update in this regime
CLIP = 50.0         # the cell clip of the reference layer

FWD_GROUPS = ("G", "I", "F", "O", "C", "H", "M", "R")
BWD_GROUPS = ("DG", "DI", "DF", "DO", "DC", "DR")      # (DH / DM are never materialised by the engine)
PARAM_NAMES = tuple(n for n, _ in param_sizes(1, 1, 1))


def x_scale(I):
    """x of the first layer ~ N(0, 1) (features); x of an inner layer (I > 40) ~ 2 N(0, 1), the size of a lower layer's r."""
    return 1.0 if I <= 40 else 2.0


def trained_params(I, C, R, seed):
    """fp32 blob in GetParams order: U[-s, s] per tensor with w_gifo_x s = 0.3 sqrt(40 / I) / x_scale(I) (0.3 at I = 40, 0.042 at
    I = 512), w_gifo_r 0.1, bias 1.0 plus +-3 (random sign per gate and cell) on the i, f and o gates, peepholes 0.3, w_r_m 0.1."""
    rng = np.random.RandomState(seed)
    sx = 0.3 * np.sqrt(40.0 / I) / x_scale(I)
    scale = {"w_gifo_x": sx, "w_gifo_r": 0.1, "bias": 1.0, "peephole_i_c": 0.3, "peephole_f_c": 0.3, "peephole_o_c": 0.3,
             "w_r_m": 0.1}
    parts = []
    for name, shp in param_sizes(I, C, R):
        t = (rng.rand(*shp) - 0.5) * 2 * scale[name]
        if name == "bias":
            t[C:] += 3.0 * np.sign(rng.rand(3 * C) - 0.5)
        parts.append(t.ravel())
    return np.concatenate(parts).astype(np.float32)


def trained_inputs(I, R, T, S, rng, od_scale=1.0):
    """x [T*S, I] ~ x_scale(I) N(0, 1) and out_diff [T*S, R] ~ od_scale N(0, 1), fp32."""
    x = (x_scale(I) * rng.randn(T * S, I)).astype(np.float32)
    od = (od_scale * rng.randn(T * S, R)).astype(np.float32)
    return x, od


def _tensors(C, S, T, out, in_diff, Y, D, state_c, state_r, corr, dparams, I, R):
    """The tensors compared per minibatch, as float64 arrays keyed by name."""
    rec = {"out": out, "state_c": state_c, "state_r": state_r}
    if in_diff is not None:
        rec["in_diff"] = in_diff
    rows = slice(S, (T + 1) * S)                                   # frames 1..T (block 0 is the carried state)
    for k, name in enumerate(FWD_GROUPS):
        lo = k * C
        hi = lo + (R if name == "R" else C)
        rec["Y" + name] = Y[rows, lo:hi]
    for name in BWD_GROUPS:
        k = FWD_GROUPS.index(name[1])
        lo = k * C
        hi = lo + (R if name == "DR" else C)
        rec[name] = D[rows, lo:hi]
    for n, v in split_blob(np.asarray(corr), I, C, R).items():
        rec["corr." + n] = v
    for n, v in split_blob(np.asarray(dparams), I, C, R).items():
        rec["dparams." + n] = v
    return {k: np.asarray(v, np.float64) for k, v in rec.items()}


# the shapes of the parity cases (tests/test_trained_regime_gpu.py), pinned on the oracles alone by tests/test_trained_regime.py; seed 3
# keeps max |dgifo| below 16 at out_diff scale 1 in every one of them (the fp16-plane products' range guard starts at 16)
SEED = 3
SHAPES = {
    "i40_s4": dict(I=40, S=4),
    "i40_s8": dict(I=40, S=8),                    # two interleaved chains
    "i40_s16": dict(I=40, S=16),                  # four
    "i512_s4": dict(I=512, S=4),                  # configs[3]'s inner layer
    "i512_s4_od2": dict(I=512, S=4, od_scale=2.0),   # ... with derivatives past the range guard's 16
    # T across the fold policy's 12 (re-pack on demand), then a reset of two streams whose c sits at +-50 (the clip fires in every
    # stream from the fifth minibatch on: ~60 frames in)
    "i40_s4_tseq": dict(I=40, S=4, Ts=(20, 14, 7, 20, 20, 20), resets=[None, None, None, None, None, [0, 1, 1, 0]]),
}
C_FULL, R_FULL, T_FULL, NMB = 800, 512, 20, 5


def shape_args(key):
    a = dict(C=C_FULL, R=R_FULL, Ts=(T_FULL,) * NMB, od_scale=1.0, resets=None, seed=SEED)
    a.update(SHAPES[key])
    return a


_LAST = {}


def _oracle_minibatch(o, x, od, T, reset, lr, momentum, want_in_diff, theta_ref):
    """One minibatch on an oracle (Reset, Propagate, Backpropagate, Update), read back as _tensors with dparams = theta - theta_ref."""
    C, S, I, R = o.C, o.S, o.I, o.R
    if reset is not None:
        o.reset(np.asarray(reset, np.int32))
    out = o.propagate(x)
    ind = o.backpropagate(x, od, momentum=momentum, want_in_diff=want_in_diff)
    o.update(lr)
    st = o.get_state()
    return _tensors(C, S, T, out, ind, o.prop_buf(), o.bprop_buf(), st[:, 4 * C:5 * C], st[:, 7 * C:], o.get_corr(),
                    o.get_params() - np.asarray(theta_ref, o.dtype), I, R)


def _engine_minibatch(engine, x, od, T, reset, lr, momentum, flags, want_in_diff, theta_ref):
    """The same minibatch on a kaldi_lstm_amd.Engine (fp32 inputs on the device), read back after the Update."""
    import torch
    I, C, R, S = engine.I, engine.C, engine.R, engine.S
    if reset is not None:
        engine.reset(list(reset))
    xd, odd = torch.from_numpy(x).cuda(), torch.from_numpy(od).cuda()
    outd = torch.empty(T * S, R, device="cuda")
    idd = torch.empty(T * S, I, device="cuda") if want_in_diff else None
    torch.cuda.synchronize()
    engine.propagate(xd, outd)
    engine.backpropagate(xd, odd, idd, momentum=momentum, flags=flags)
    engine.update(lr)
    engine.synchronize()
    cs, rs = engine.get_state()
    return _tensors(C, S, T, outd.cpu().numpy(), idd.cpu().numpy() if want_in_diff else None, engine.activations(0),
                    engine.activations(1), cs, rs, engine.get_corr(), engine.get_params().astype(np.float64) - theta_ref, I, R)


def oracle_runs(I, C, R, S, Ts, lr=LR, od_scale=1.0, resets=None, seed=SEED, want_in_diff=True, momentum=MOMENTUM, threads=8):
    """The fp32 and fp64 oracle sides of run_vs_fp64: one dict per minibatch, tensor name -> {"f32", "f64"}.  The last call's result
    is kept (tests that run several engines on one shape pay for the oracles once)."""
    key = (I, C, R, S, tuple(Ts), lr, od_scale, None if resets is None else tuple(map(lambda r: None if r is None else tuple(r), resets)),
           seed, want_in_diff, momentum)
    if _LAST.get("key") == key:
        return _LAST["recs"]
    _LAST.clear()
    p0 = trained_params(I, C, R, seed + 1)
    rng = np.random.RandomState(seed)
    o32, o64 = Oracle(I, C, R, S, np.float32, threads=threads), Oracle(I, C, R, S, np.float64, threads=threads)
    o32.set_params(p0)
    o64.set_params(p0.astype(np.float64))
    recs = []
    for k, T in enumerate(Ts):
        x, od = trained_inputs(I, R, T, S, rng, od_scale)
        sides = {}
        for name, o in (("f32", o32), ("f64", o64)):
            sides[name] = _oracle_minibatch(o, x, od, T, None if resets is None else resets[k], lr, momentum, want_in_diff, p0)
        recs.append({t: {s: v[t] for s, v in sides.items()} for t in sides["f64"]})
    _LAST.update(key=key, recs=recs)
    return recs


def run_vs_fp64(engine, I, C, R, S, Ts, lr=LR, od_scale=1.0, resets=None, seed=SEED, flags=0, want_in_diff=True,
                momentum=MOMENTUM, threads=8, on_step=None):
    """len(Ts) chained minibatches (Propagate, Backpropagate, Update; c / r carried) on three sides -- `engine` (a kaldi_lstm_amd.Engine
    with its options set, or None), Oracle(float32) and Oracle(float64) -- each evolving its own parameters, momentum and state from the
    same fp32 parameters trained_params(I, C, R, seed + 1), on inputs trained_inputs(...) drawn from RandomState(seed).  resets[k]:
    per-stream flags applied before minibatch k (or None); flags: the engine's backpropagate flags (2 = KLSTM_BPTT_FUSE_UPDATE).
    Everything is read back after the Update.  on_step(k, engine) runs after minibatch k (counters).  Returns one dict per minibatch:
    tensor name -> {"eng", "f32", "f64"}; the parameters enter as dparams.* = theta_k - theta_0 (theta_0 is shared by all sides and
    would hide an Update error)."""
    recs = oracle_runs(I, C, R, S, Ts, lr, od_scale, resets, seed, want_in_diff, momentum, threads)
    if engine is None:
        return recs
    p0 = trained_params(I, C, R, seed + 1)
    rng = np.random.RandomState(seed)
    engine.set_params(p0)
    out = []
    for k, T in enumerate(Ts):
        x, od = trained_inputs(I, R, T, S, rng, od_scale)
        eng = _engine_minibatch(engine, x, od, T, None if resets is None else resets[k], lr, momentum, flags, want_in_diff,
                                p0.astype(np.float64))
        if on_step is not None:
            on_step(k, engine)
        out.append({t: dict(recs[k][t], eng=eng[t]) for t in recs[k]})
    return out


def relerr(a, b):
    """max |a - b| / max |b| (b: the fp64 truth)."""
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / (np.abs(b).max() + 1e-30))


def saturated_fraction(rec, tol=0.02):
    """Fraction of the i / f / o gate values (fp64) within tol of 0 or 1."""
    g = np.concatenate([rec["Y" + n]["f64"].ravel() for n in ("I", "F", "O")])
    return float(np.mean((g < tol) | (g > 1 - tol)))


def clipped_count(c):
    """Entries of a C group at exactly +-CLIP."""
    return int(np.count_nonzero(np.abs(c) == CLIP))


def max_dgifo(rec):
    return max(float(np.abs(rec[n]["f64"]).max()) for n in ("DG", "DI", "DF", "DO"))


def w_rm_max(I, C, R, params):
    """max |W_gifo_r W_r_m| of a GetParams-order blob (the folded recurrence of the persistent forward chain)."""
    p = split_blob(np.asarray(params, np.float64), I, C, R)
    return float(np.abs(p["w_gifo_r"] @ p["w_r_m"]).max())


# ---- bf16 operand mode: the fp64 oracle on bf16-rounded weights as the yardstick, re-anchored on the engine every minibatch ----
#
# Chained over minibatches, rounding the weights to bf16 is a chaotic perturbation in this regime: at 512/1024/512 x 32 the fp64
# oracle on bf16 weights (B) drifts from the one on the fp32 weights (A) from relerr 8e-3 to 0.11 in `out` and 2.6e-2 to 0.5 in
# in_diff within five minibatches -- a ratio bar over carried trajectories would let anything pass.  run_bf16_vs_fp64() therefore
# starts A and B from the ENGINE's parameters, momentum buffers and carried (c, r) before every minibatch: what is compared is one
# minibatch's worth of bf16 error, which stays flat (out 4-8e-3, in_diff 1-3e-2) while the engine walks the saturated trajectory.

BF16_WEIGHTS = ("w_gifo_x", "w_gifo_r", "w_r_m")


def bf16_rne(a):
    """IEEE round-to-nearest-even of fp32 values to bf16 (as fp32): the format's definition, not a choice of this build."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def round_weights_bf16(theta, I, C, R):
    """theta (fp32 blob) with the three weight matrices rounded to bf16; bias and peepholes unchanged.  Those two enter only the
    engine's fp32 elementwise cell math, so rounding them (as the one-minibatch budget test of tests/test_engine_gpu.py does with the
    whole blob) would add a perturbation the engine does not make and loosen the bar by it."""
    out = np.array(theta, np.float32, copy=True)
    parts = split_blob(out, I, C, R)               # (views into out)
    for n in BF16_WEIGHTS:
        parts[n][...] = bf16_rne(parts[n])
    return out


def state_row(c, r, C, R, dtype):
    """An oracle state row [S, 7C + R] holding only c (column group C) and r (group R): all the engine returns, and all a
    minibatch reads from the carried block (tests/test_trained_regime.py checks that bit-exactly)."""
    S = c.shape[0]
    st = np.zeros((S, 7 * C + R), dtype)
    st[:, 4 * C:5 * C] = c
    st[:, 7 * C:] = r
    return st


def clipped_streams(c):
    """Reset flags for every other stream (the 2nd, 4th, ...) of those whose carried c has an entry at +-CLIP: by the time the clip
    fires, every stream of 1024 cells has such an entry, and the streams left alone keep the clip firing after the Reset."""
    hit = np.flatnonzero((np.abs(np.asarray(c)) == CLIP).any(axis=1))
    flags = np.zeros(np.shape(c)[0], np.int32)
    flags[hit[1::2]] = 1
    return flags


def run_bf16_vs_fp64(engine, I, C, R, S, Ts, lr=LR, od_scale=1.0, resets=None, seed=SEED, flags=0, want_in_diff=True,
                     momentum=MOMENTUM, threads=8, on_step=None, with_f32=False):
    """len(Ts) minibatches (Propagate, Backpropagate, Update) from the fp32 parameters trained_params(I, C, R, seed + 1), on inputs
    trained_inputs(...) drawn from RandomState(seed).  The trajectory is the engine's (`engine`: a kaldi_lstm_amd.Engine with its
    options set): before minibatch k its parameters theta_k, momentum buffers and carried (c, r) are read and loaded into two fp64
    oracles -- "A" with theta_k as it is, "B" with round_weights_bf16(theta_k) -- and, with_f32, an fp32 oracle "f32" with theta_k;
    then all sides run the same minibatch.  engine None: the anchor is A itself (its parameters, momentum and state after each
    minibatch, rounded to fp32 as an engine would hold them).  resets[k]: per-stream flags applied before minibatch k on every side,
    None, or "clipped" (clipped_streams() of the anchor's c).  on_step(k, engine) runs after the engine's minibatch k.
    Returns one dict per minibatch: tensor name -> {"eng" (with an engine), "A", "B"[, "f32"]}; dparams.* = theta after - theta
    before this minibatch on each side (B: from its rounded theta_k); plus "_resets": the flags applied (or None)."""
    p0 = trained_params(I, C, R, seed + 1)
    rng = np.random.RandomState(seed)
    oracles = [("A", Oracle(I, C, R, S, np.float64, threads=threads)), ("B", Oracle(I, C, R, S, np.float64, threads=threads))]
    if with_f32:
        oracles.append(("f32", Oracle(I, C, R, S, np.float32, threads=threads)))
    theta, corr = p0, np.zeros_like(p0)
    c, r = np.zeros((S, C), np.float32), np.zeros((S, R), np.float32)
    if engine is not None:
        engine.set_params(p0)
    recs = []
    for k, T in enumerate(Ts):
        x, od = trained_inputs(I, R, T, S, rng, od_scale)
        reset = None if resets is None else resets[k]
        if isinstance(reset, str):
            assert reset == "clipped", reset
            reset = clipped_streams(c)
        sides = {}
        for name, o in oracles:
            th = round_weights_bf16(theta, I, C, R) if name == "B" else theta
            o.set_params(th.astype(o.dtype))
            o.set_corr(corr.astype(o.dtype))
            o.set_state(state_row(c, r, C, R, o.dtype))
            sides[name] = _oracle_minibatch(o, x, od, T, reset, lr, momentum, want_in_diff, th)
        if engine is not None:
            sides["eng"] = _engine_minibatch(engine, x, od, T, reset, lr, momentum, flags, want_in_diff, theta.astype(np.float64))
            if on_step is not None:
                on_step(k, engine)
            theta, corr = engine.get_params(), engine.get_corr()
            c, r = engine.get_state()
        else:
            oa = oracles[0][1]
            st = oa.get_state()
            theta, corr = oa.get_params().astype(np.float32), oa.get_corr().astype(np.float32)
            c, r = st[:, 4 * C:5 * C].astype(np.float32), st[:, 7 * C:].astype(np.float32)
        rec = {t: {s: v[t] for s, v in sides.items()} for t in sides["A"]}
        rec["_resets"] = reset
        recs.append(rec)
    return recs


# the shapes of the bf16 cases (tests/test_trained_regime_bf16_gpu.py), pinned on the oracles alone by tests/test_trained_regime.py.
# 1024 cells keep the recipe of the 800-cell shapes: max |dgifo| reaches ~22 in the first minibatch at I = 512, which is fine here --
# the bf16 operand mode has no fp16 range guard.
BF16_SHAPES = {
    "i512_c1024_s32": dict(I=512, C=1024, S=32),        # BASELINE configs[4]'s inner layer: per-XCD chains both ways
    "i40_c1024_s32": dict(I=40, C=1024, S=32),          # ... its bottom layer (fp32 batched x term)
    "i512_c1024_s16": dict(I=512, C=1024, S=16),        # per-XCD chains, fewer streams per group
    "i40_c800_s32": dict(I=40, C=800, S=32),            # per-XCD chains at C != 1024: cell-less slots
    "i512_c800_s32": dict(I=512, C=800, S=32),
    # T S = 640, 256 (the threshold of both persistent launches and of the bf16 gradient tiles), 224 (below it: launch per step),
    # then a Reset of half the streams whose c sits at +-50 before the last minibatch (six minibatches: the clip fires ~60 frames in)
    "i512_c1024_s32_tseq": dict(I=512, C=1024, S=32, Ts=(20, 8, 7, 20, 20, 20),
                                resets=[None, None, None, None, None, "clipped"]),
    "i40_c800_s4": dict(I=40, C=800, S=4),              # "bf16" = 2: forced bf16 operands on the launch-per-step kernels
}


def bf16_shape_args(key):
    a = dict(R=R_FULL, Ts=(T_FULL,) * NMB, od_scale=1.0, resets=None, seed=SEED)
    a.update(BF16_SHAPES[key])
    return a
