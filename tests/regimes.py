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
            if resets is not None and resets[k] is not None:
                o.reset(np.asarray(resets[k], np.int32))
            out = o.propagate(x)
            ind = o.backpropagate(x, od, momentum=momentum, want_in_diff=want_in_diff)
            o.update(lr)
            st = o.get_state()
            sides[name] = _tensors(C, S, T, out, ind, o.prop_buf(), o.bprop_buf(), st[:, 4 * C:5 * C], st[:, 7 * C:],
                                   o.get_corr(), o.get_params() - p0.astype(o.dtype), I, R)
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
    import torch
    p0 = trained_params(I, C, R, seed + 1)
    rng = np.random.RandomState(seed)
    engine.set_params(p0)
    out = []
    for k, T in enumerate(Ts):
        x, od = trained_inputs(I, R, T, S, rng, od_scale)
        if resets is not None and resets[k] is not None:
            engine.reset(list(resets[k]))
        xd, odd = torch.from_numpy(x).cuda(), torch.from_numpy(od).cuda()
        outd = torch.empty(T * S, R, device="cuda")
        idd = torch.empty(T * S, I, device="cuda") if want_in_diff else None
        torch.cuda.synchronize()
        engine.propagate(xd, outd)
        engine.backpropagate(xd, odd, idd, momentum=momentum, flags=flags)
        engine.update(lr)
        engine.synchronize()
        cs, rs = engine.get_state()
        eng = _tensors(C, S, T, outd.cpu().numpy(), idd.cpu().numpy() if want_in_diff else None, engine.activations(0),
                       engine.activations(1), cs, rs, engine.get_corr(), engine.get_params().astype(np.float64) - p0, I, R)
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
