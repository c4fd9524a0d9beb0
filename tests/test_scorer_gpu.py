"""Batched scoring on the device: klstm_propagate_inference against klstm_propagate (bit for bit), the pack and output kernels against
numpy, and the whole scorer (include/klstm_scorer.hpp through tests/cpp/scorer_test) against the per-utterance path -- the oracle chain
time_shift -> Oracle(S = 1) -> affine -> log-softmax - prior, and the nnet-forward workalike on the converted standard model."""
import numpy as np
import pytest
import torch

import kaldi_lstm_amd as k
from oracle import components as oc
from oracle.oracle import Oracle, make_params
from tests import kaldi_fmt
from tests.margins import bound
from tests.test_component import run as run_component
from tests.test_scorer import run

pytestmark = pytest.mark.gpu


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / (np.abs(b).max() + 1e-30))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. forward only = forward, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(40, 800, 512), (512, 800, 512)], ids=["40-800-512", "512-800-512"])
@pytest.mark.parametrize("S", [1, 4, 5, 8, 12, 16])
def test_propagate_inference_is_bit_identical(shape, S):
    I, C, R = shape
    p = make_params(I, C, R, scale=0.1, seed=S)
    rng = np.random.RandomState(S)
    ea, eb = k.Engine(I, C, R, S), k.Engine(I, C, R, S)
    ea.set_params(p); eb.set_params(p)
    for T in (8, 20, 50):
        for chunk in range(3):
            flags = [1] * S if chunk == 0 else list(rng.randint(0, 2, S))
            ea.reset(flags); eb.reset(flags)
            x = torch.from_numpy(rng.uniform(-1, 1, (T * S, I)).astype(np.float32)).cuda()
            oa, ob = torch.empty(T * S, R, device="cuda"), torch.full((T * S, R), float("nan"), device="cuda")
            ea.propagate(x, oa)
            eb.propagate_inference(x, ob)
            ea.synchronize(); eb.synchronize()
            assert torch.equal(oa, ob), (T, chunk, float((oa - ob).abs().max()))
            (ca, ra), (cb, rb) = ea.get_state(), eb.get_state()
            assert np.array_equal(ca, cb) and np.array_equal(ra, rb), (T, chunk)
    # nothing is kept for a BPTT after a forward-only pass
    x = torch.from_numpy(rng.uniform(-1, 1, (8 * S, I)).astype(np.float32)).cuda()
    ob = torch.empty(8 * S, R, device="cuda")
    eb.propagate_inference(x, ob)
    with pytest.raises(k.KlstmError) as ei:
        eb.backpropagate(x, torch.zeros(8 * S, R, device="cuda"))
    assert ei.value.status == 3
    ea.propagate(x, torch.empty_like(ob))
    # alternating the two calls keeps the carried state continuous
    for j in range(4):
        x = torch.from_numpy(rng.uniform(-1, 1, (20 * S, I)).astype(np.float32)).cuda()
        oa, ob = torch.empty(20 * S, R, device="cuda"), torch.empty(20 * S, R, device="cuda")
        ea.propagate(x, oa)
        (eb.propagate if j % 2 else eb.propagate_inference)(x, ob)
        ea.synchronize(); eb.synchronize()
        assert torch.equal(oa, ob), j
    eb.backpropagate(x, torch.zeros(20 * S, R, device="cuda"))     # (after a training propagate it works again)
    eb.synchronize()
    # the forward-only instances ran where they are dispatched (klstm_persist.hip persist_fwd_has_inference), and only there
    n_inf = eb.profile_query("fwd_inference_launches")[1]
    if (I == 40 and S >= 5) or (I == 512 and S <= 8):
        assert n_inf > 0
    else:
        assert n_inf == 0
    assert ea.profile_query("fwd_inference_launches")[1] == 0
    ea.close(); eb.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the pack and output kernels
# ---------------------------------------------------------------------------------------------------------------------------------
def pack_numpy(feats, desc, T, shift):
    S, dim = desc.shape[0], feats.shape[1]
    out = np.zeros((T, S, dim), np.float32)
    for s, (off, n, start) in enumerate(desc):
        if n <= 0:
            continue
        src = np.clip(start + np.arange(T) + shift, 0, n - 1)
        out[:, s] = feats[off + src]
    return out.reshape(T * S, dim)


@pytest.mark.parametrize("dim", [40, 13])
@pytest.mark.parametrize("shift", [0, 5, -2])
def test_pack_streams_is_the_gather(dim, shift):
    rng = np.random.RandomState(dim + shift)
    lens = [23, 3, 57, 1, 40]
    off = np.concatenate([[0], np.cumsum(lens)])
    feats = rng.randn(off[-1], dim).astype(np.float32)
    T, S = 20, 7
    desc = np.array([[off[0], 23, 0], [off[1], 3, 0], [off[2], 57, 40], [0, 0, 0], [off[3], 1, 0], [off[4], 40, 20], [off[2], 57, 20]],
                    np.int32)                                       # starts, continuations, a row past the end, an idle stream
    out = torch.full((T * S, dim), float("nan"), device="cuda")
    reset = torch.full((S,), 7, dtype=torch.int32, device="cuda")
    k.pack_streams(torch.from_numpy(feats).cuda(), torch.from_numpy(desc).cuda(), T, shift, out, reset)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), pack_numpy(feats, desc, T, shift))
    assert reset.cpu().tolist() == [1, 1, 0, 1, 1, 0, 0]


def log_softmax64(a):
    a = a.astype(np.float64)
    z = a - a.max(1, keepdims=True)
    return z - np.log(np.exp(z).sum(1, keepdims=True))


@pytest.mark.parametrize("cols", [16624, 1000, 11])
@pytest.mark.parametrize("mode", [k.SCORE_POSTERIOR, k.SCORE_LOGPOST, k.SCORE_LOGLIKE], ids=["post", "logpost", "loglike"])
def test_log_softmax_scatter(cols, mode):
    rng = np.random.RandomState(cols + mode)
    rows, nout = 48, 40
    a = (3.0 * rng.randn(rows, cols)).astype(np.float32)
    a[5] += 30.0 * (np.arange(cols) == 3)                          # one very confident row: tail posteriors underflow in fp32
    dst = rng.permutation(nout + 20)[:rows] - 20                    # some rows padding (< 0), the rest a permutation of output rows
    dst = np.where(dst < 0, -1, dst).astype(np.int32)
    log_prior = np.log(rng.dirichlet(np.ones(cols))).astype(np.float32)
    ps = 0.8
    out = torch.full((nout, cols), 123.0, device="cuda")
    k.log_softmax_scatter(torch.from_numpy(a).cuda(), torch.from_numpy(dst).cuda(), out, mode,
                          torch.from_numpy(log_prior).cuda(), ps)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    lp = log_softmax64(a)
    ref = np.exp(lp) if mode == k.SCORE_POSTERIOR else lp - ps * log_prior.astype(np.float64) if mode == k.SCORE_LOGLIKE else lp
    on = dst >= 0
    g, r = got[dst[on]], ref[on]
    assert np.all(np.isfinite(g))
    bars = {k.SCORE_POSTERIOR: 1e-6, k.SCORE_LOGPOST: 5e-7, k.SCORE_LOGLIKE: 1e-6}       # measured 1.1e-7, 5.0e-8, 1.3e-7
    bound(rel(g, r), bars[mode], "scores")
    untouched = np.setdiff1d(np.arange(nout), dst[on])
    assert len(untouched) > 0 and np.all(got[untouched] == 123.0)    # rows nobody names keep the sentinel
    if mode == k.SCORE_POSTERIOR:                                   # the posterior is klstm_softmax's arithmetic, bit for bit
        post = torch.empty(rows, cols, device="cuda")
        k.softmax(torch.from_numpy(a).cuda(), post)
        torch.cuda.synchronize()
        assert np.array_equal(post.cpu().numpy()[on], g)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the scorer against the per-utterance path
# ---------------------------------------------------------------------------------------------------------------------------------
SMALL = dict(I=8, C=16, R=8, NPDF=11, layers=1, nutt=40, lmin=1, lmax=60, scale=0.3)
BIG = dict(I=40, C=800, R=512, NPDF=16624, layers=2, nutt=20, lmin=10, lmax=90, scale=0.1)     # configs[3] size


def make_model(cfg, seed):
    rng = np.random.RandomState(seed)
    I, C, R, NPDF, sc = cfg["I"], cfg["C"], cfg["R"], cfg["NPDF"], cfg["scale"]
    flats = [make_params(I if l == 0 else R, C, R, scale=sc, seed=seed + 1 + l) for l in range(cfg["layers"])]
    if cfg is BIG:
        flats = [rng.uniform(-0.1, 0.1, f.size).astype(np.float32) for f in flats]          # params U[-0.1, 0.1]
        W, b = rng.uniform(-0.1, 0.1, (NPDF, R)).astype(np.float32), rng.uniform(-0.1, 0.1, NPDF).astype(np.float32)
    else:
        W, b = (sc * rng.randn(NPDF, R)).astype(np.float32), (0.1 * rng.randn(NPDF)).astype(np.float32)
    return flats, W, b


def oracle_scores(cfg, flats, W, b, utts, shift, log_prior, ps):
    """per utterance: time_shift -> Oracle(S = 1) per layer -> affine -> log-softmax - prior (float64 behind the LSTM)"""
    I, C, R = cfg["I"], cfg["C"], cfg["R"]
    lstms = []
    for l, f in enumerate(flats):
        o = Oracle(I if l == 0 else R, C, R, 1, np.float32, threads=8)
        o.set_params(f)
        lstms.append(o)
    outs = []
    for x in utts:
        h = oc.time_shift(x, shift)
        for o in lstms:
            o.reset([1])
            h = o.propagate(h)
        a = h.astype(np.float64) @ W.T.astype(np.float64) + b
        outs.append(log_softmax64(a) - ps * log_prior.astype(np.float64))
    return outs


def score(tmp_path, model, utts, S, T, mode, delay, log_prior=None, ps=1.0, tag=""):
    feats = np.concatenate(utts).astype(np.float32)
    feats.tofile(tmp_path / "x.raw")
    lp = "none"
    if log_prior is not None:
        log_prior.astype(np.float32).tofile(tmp_path / "lp.raw")
        lp = tmp_path / "lp.raw"
    out = tmp_path / ("y%s.raw" % tag)
    r = run("score", model, tmp_path / "x.raw", ",".join(str(len(u)) for u in utts), S, T, mode, delay, lp, ps, out)
    head = r.stdout.split()
    assert head[0] == "OK" and int(head[1]) == len(utts)
    y = np.fromfile(out, np.float32).reshape(-1, int(head[2]))
    return np.split(y, np.cumsum([len(u) for u in utts])[:-1])


@pytest.mark.parametrize("cfg", [SMALL, BIG], ids=["small", "configs3"])
def test_scorer_equals_per_utterance_path(tmp_path, cfg):
    seed, shift, ps = 11, 5, 0.7
    flats, W, b = make_model(cfg, seed)
    I, C, R, NPDF = cfg["I"], cfg["C"], cfg["R"], cfg["NPDF"]
    rng = np.random.RandomState(seed)
    lens = rng.randint(cfg["lmin"], cfg["lmax"] + 1, cfg["nutt"])
    utts = [rng.uniform(-1, 1, (n, I)).astype(np.float32) for n in lens]
    log_prior = np.log(rng.dirichlet(np.ones(NPDF))).astype(np.float32)
    google = [("transmit", I)] + [("lstm_streams", f, I if l == 0 else R, C, R, 4) for l, f in enumerate(flats)] + [("affine", W, b), ("softmax", NPDF)]
    (tmp_path / "g.bin").write_bytes(kaldi_fmt.nnet_binary(google))
    run("convert", tmp_path / "g.bin", shift, 1, tmp_path / "s.bin")
    ref = oracle_scores(cfg, flats, W, b, utts, shift, log_prior, ps)
    refcat = np.concatenate(ref)
    bar = 2e-6 if cfg is SMALL else 7e-6              # measured 1.9e-7 / 7.4e-7 (fp32 chain against the fp32 oracle + float64 tail)
    bar_st = 1.5e-6 if cfg is SMALL else 6e-6         # measured 1.8e-7 / 6.4e-7 (S = 16 runs other kernels than S = 1 / 4: rounding only)
    got = {}
    for form, model, delay in (("google", tmp_path / "g.bin", shift), ("standard", tmp_path / "s.bin", "none")):
        for S in (1, 4, 16):
            y = score(tmp_path, model, utts, S, 20, "loglike", delay, log_prior, ps, tag="%s%d" % (form, S))
            assert [len(u) for u in y] == list(lens)
            got[(form, S)] = np.concatenate(y)
            bound(rel(got[(form, S)], refcat), bar, "loglike %s S=%d vs oracle" % (form, S))
    # chunk length does not change the result beyond fp32 rounding; the stream count neither
    y50 = np.concatenate(score(tmp_path, tmp_path / "s.bin", utts, 4, 50, "loglike", "none", log_prior, ps, tag="t50"))
    base = got[("standard", 4)]
    bound(rel(y50, base.astype(np.float64)), bar_st, "T=50 vs T=20")
    for key, y in got.items():
        bound(rel(y, base.astype(np.float64)), bar_st, "%s S=%d vs standard S=4" % key)
    # posteriors against the nnet-forward workalike on the converted (standard) model, one utterance per call
    post = score(tmp_path, tmp_path / "s.bin", utts, 16, 20, "post", "none", tag="post")
    for u in (0, 1, len(utts) - 1):
        utts[u].tofile(tmp_path / "u.raw")
        out = run_component("nnet_forward", tmp_path / "s.bin", tmp_path / "u.raw", len(utts[u]), tmp_path / "f.raw").stdout.split()
        assert out == ["OK", str(len(utts[u])), str(NPDF)]
        fw = np.fromfile(tmp_path / "f.raw", np.float32).reshape(len(utts[u]), NPDF)
        bound(float(np.abs(post[u] - fw).max()), 6e-9, "posterior vs nnet_forward")        # measured 0 / 6.4e-10
