"""The numpy twin of the knlm_* entries (include/klstm_nlm.h, which defines every quantity; kaldi-lstm_amd/csrc/klstm_ctc_nlm.hip;
DESIGN.md 4u), host only: rescoring of CTC n-best lists with an LSTM language model.  The lists are read under the contract of
klstm_ctc_nbest_rescore (tests/ctc_rescore_ref.py).  The net -- [embedding] -> LSTMP layers -> Affine -- runs the oracle
(oracle/lstmp_oracle.c) and oracle/components.py as tests/nnet_twins.py does: in float64 by default, in float32 with dtype=np.float32
(the LSTM layers and the Affine at float32: the error a float32 implementation of the same net may have).  lp of a row is formed in
float64 from the row the net gave and rounded to float once; the sums and z are the device's operations in the device's order.
tests/test_ctc_nlm.py holds this twin against an independent brute force."""
import collections

import numpy as np

from oracle import components as comp
from oracle.oracle import Oracle

TOTALS = 8
F32 = np.float32

# layers: [(flat parameters, I, C, R)]; W [V, R], b [V]: the last Affine; embed: None or (We [D, V], be [D]); bos, eos: classes (eos < 0: none)
Lm = collections.namedtuple("Lm", "layers W b embed bos eos")


def classes(lm):
    return int(lm.W.shape[0])


def well_formed(hyp, hyp_len, count, logp, K, max_len):
    """-> state [S, N]: 0 unlisted, 1 dropped, 3 well formed (forbidden, 2, is the ranking's to say)"""
    S, N, stride = hyp.shape
    st = np.zeros((S, N), np.int32)
    for s in range(S):
        c = int(count[s])
        if c < 0 or c > N:
            continue
        for q in range(c):
            n = int(hyp_len[s, q])
            ok = bool(np.isfinite(F32(logp[s, q]))) and 0 <= n <= min(stride, max_len)
            ok = ok and all(0 <= t < K for t in hyp[s, q, :n].tolist())
            st[s, q] = 3 if ok else 1
    return st


def inputs_of(toks, bos, eos):
    """the classes that go in, one per position"""
    return [bos] + list(toks) if eos >= 0 else ([bos] + list(toks))[:len(toks)]


def targets_of(toks, eos):
    return list(toks) + ([eos] if eos >= 0 else [])


def input_row(lm, x):
    """one engine input row, float32: the device's bits"""
    if lm.embed is None:
        r = np.zeros(classes(lm), F32)
        r[x] = 1
        return r
    We, be = lm.embed
    return (We[:, x].astype(F32) + be.astype(F32)).astype(F32)


def pack_rows(hyp, hyp_len, count, logp, K, lm, first_entry, E, T, t0, max_len=None):
    """the chunk knlm_pack writes: [T * E, V or D] float32"""
    S, N, stride = hyp.shape
    max_len = min(1023, stride) if max_len is None else max_len
    st = well_formed(hyp, hyp_len, count, logp, K, max_len).ravel()
    cols = classes(lm) if lm.embed is None else lm.embed[0].shape[0]
    out = np.zeros((T * E, cols), F32)
    for e in range(E):
        se = first_entry + e
        if se >= S * N or st[se] != 3:
            continue
        toks = hyp.reshape(S * N, stride)[se, :hyp_len.ravel()[se]].tolist()
        xs = inputs_of(toks, lm.bos, lm.eos)
        for t in range(T):
            if t0 + t < len(xs):
                out[t * E + e] = input_row(lm, xs[t0 + t])
    return out


def logits(lm, seqs, dtype=np.float64):
    """the rows of the last Affine for input class sequences `seqs`, each from zero state -> a list of [len, V] arrays of dtype.  The
    sequences run as the streams of one oracle per layer, padded with zero rows behind their ends (which nothing before them sees)"""
    n, P = len(seqs), max([len(x) for x in seqs] + [1])
    cols = classes(lm) if lm.embed is None else lm.embed[0].shape[0]
    x = np.zeros((P * n, cols), dtype)
    for s, xs in enumerate(seqs):
        for p, c in enumerate(xs):
            x[p * n + s] = input_row(lm, c)
    for flat, I, C, R in lm.layers:
        o = Oracle(I, C, R, n, dtype)
        o.set_params(np.asarray(flat, dtype))
        o.reset(np.ones(n, np.int32))
        x = o.propagate(x)
    a = comp.affine_propagate(x, lm.W.astype(dtype), lm.b.astype(dtype))
    return [a[np.arange(len(xs)) * n + s] for s, xs in enumerate(seqs)]


def row_logp64(a, tgt):
    """(a[tgt] - max) - log(sum exp(a - max)) in float64 of a row of any dtype"""
    a = np.asarray(a, np.float64)
    with np.errstate(all="ignore"):
        m = a.max() if not np.isnan(a).any() else np.nan
        return (a[tgt] - m) - np.log(np.exp(a - m).sum())


def score_entries(hyp, hyp_len, count, logp, K, lm, max_len=None, dtype=np.float64):
    """-> acc [S, N] float64 (nlm_logp: the sum over p ascending of double(float(lp_p)); 0 where the entry is not well formed),
    positions [S, N] int32, exact [S, N] float64 (the same sum without the rounding of lp to float)"""
    hyp, hyp_len, count = np.asarray(hyp), np.asarray(hyp_len), np.asarray(count)
    S, N, stride = hyp.shape
    max_len = min(1023, stride) if max_len is None else max_len
    st = well_formed(hyp, hyp_len, count, logp, K, max_len)
    acc, exact, pos = np.zeros((S, N)), np.zeros((S, N)), np.zeros((S, N), np.int32)
    idx = [(s, q) for s in range(S) for q in range(N) if st[s, q] == 3]
    toks = [hyp[s, q, :hyp_len[s, q]].tolist() for s, q in idx]
    rows = logits(lm, [inputs_of(t, lm.bos, lm.eos) for t in toks], dtype) if idx else []
    for (s, q), t, a in zip(idx, toks, rows):
        v, x = np.float64(0.0), np.float64(0.0)
        for p, tgt in enumerate(targets_of(t, lm.eos)):
            lp = row_logp64(a[p], tgt)
            with np.errstate(all="ignore"):
                v = v + np.float64(F32(lp))
                x = x + lp
        acc[s, q], exact[s, q], pos[s, q] = v, x, len(targets_of(t, lm.eos))
    return acc, pos, exact


def rank(hyp, hyp_len, count, logp, K, acc, has_eos, am_scale=1.0, nlm_scale=1.0, unit_bonus=0.0, errors=None, max_len=None, out_n=None,
         out_stride=None):
    """knlm_rank -> dict of numpy arrays named as the C entry names them, plus totals [8] (what ONE call adds), z64 [S, N] (nan: not
    ranked), status [S]"""
    hyp, hyp_len, count = np.asarray(hyp), np.asarray(hyp_len), np.asarray(count)
    logp = np.asarray(logp, dtype=F32)
    S, N, stride = hyp.shape
    max_len = min(1023, stride) if max_len is None else max_len
    out_n = N if out_n is None else out_n
    out_stride = max(min(stride, max_len), 1) if out_stride is None else out_stride
    am, ns, ub = (np.float64(F32(v)) for v in (am_scale, nlm_scale, unit_bonus))
    st = well_formed(hyp, hyp_len, count, logp, K, max_len)
    n1 = max(out_n, 1)
    o = dict(order=np.full((S, N), -1, np.int32), live_count=np.zeros(S, np.int32), score=np.full((S, N), -np.inf, F32),
             nlm_logp=np.full((S, N), -np.inf, F32), units=np.zeros((S, N), np.int32), z64=np.full((S, N), np.nan), status=[],
             out_hyp=np.zeros((S, n1, out_stride), np.int32), out_len=np.zeros((S, n1), np.int32), out_count=np.zeros(S, np.int32),
             out_score=np.full((S, n1), -np.inf, F32), out_errors=np.full((S, n1), -1, np.int32))
    tot = np.zeros(TOTALS)
    for s in range(S):
        c = int(count[s])
        if c < 0 or c > N:
            o["status"].append("rejected")
            tot[1] += 1
            continue
        z = {}
        for q in range(c):
            if st[s, q] != 3:
                tot[2] += 1
                continue
            n = int(hyp_len[s, q])
            o["units"][s, q] = n
            tot[7] += n + (1 if has_eos else 0)
            if not np.isfinite(acc[s, q]):
                tot[3] += 1
                continue
            v = am * np.float64(logp[s, q])
            v = v + ns * np.float64(acc[s, q])
            v = v + ub * np.float64(n)
            z[q] = v + np.float64(0.0)
            o["z64"][s, q], o["score"][s, q], o["nlm_logp"][s, q] = z[q], z[q], acc[s, q]
        ranked = sorted(z, key=lambda q: (-z[q], q))
        o["live_count"][s] = len(ranked)
        o["order"][s, :len(ranked)] = ranked
        if out_n >= 1:
            o["out_count"][s] = min(len(ranked), out_n)
            for r, q in enumerate(ranked[:out_n]):
                n = int(hyp_len[s, q])
                o["out_hyp"][s, r, :n], o["out_len"][s, r], o["out_score"][s, r] = hyp[s, q, :n], n, z[q]
                if errors is not None:
                    o["out_errors"][s, r] = errors[s, q]
        if not ranked:
            o["status"].append("idle")
            tot[1] += 1
            continue
        o["status"].append("done")
        tot[0] += 1
        tot[4] += ranked[0] != 0
        if errors is not None:
            tot[5] += int(errors[s, 0])
            tot[6] += int(errors[s, ranked[0]])
    o["totals"] = tot
    return o


def rescore(hyp, hyp_len, count, logp, K, lm, max_len=None, dtype=np.float64, **kw):
    """the whole second pass: score_entries, then rank.  -> the dict of rank plus acc, positions, exact"""
    acc, pos, exact = score_entries(hyp, hyp_len, count, logp, K, lm, max_len, dtype)
    o = rank(hyp, hyp_len, count, logp, K, acc, lm.eos >= 0, max_len=max_len, **kw)
    o.update(acc=acc, positions=pos, exact=exact)
    return o


def min_gap(o):
    """the smallest difference between adjacent ranked z over all streams"""
    g = np.inf
    for s in range(len(o["live_count"])):
        z = o["z64"][s, o["order"][s, :o["live_count"][s]]]
        for a, b in zip(z[:-1], z[1:]):
            g = min(g, a - b)
    return g


# ------------------------------------------------------------------------------------------------------------------------------------
# the inputs of the tests (host and GPU)
# ------------------------------------------------------------------------------------------------------------------------------------
def make_lm(K, V, bos, eos, n_lstm=1, C=16, R=8, D=None, seed=3, scale=0.3):
    """a random LM from tests/nnet_twins.make_stack, parameters float32; D: the rows of an embedding (None: one-hot input)"""
    from tests.nnet_twins import make_stack
    I = V if D is None else D
    lstm, W, b = make_stack((I, C, R, n_lstm, V), 1, seed, np.float32, scale)
    layers = [(lstm[l], I if l == 0 else R, C, R) for l in range(n_lstm)]
    embed = None
    if D is not None:
        rng = np.random.RandomState(seed + 100)
        embed = (((rng.rand(D, V) - 0.5) * 2).astype(F32), ((rng.rand(D) - 0.5) * 0.2).astype(F32))
    return Lm(layers, W, b, embed, bos, eos)


def poisoned_lists(K=6, max_len=7, poison=10 ** 6, seed=0, more_streams=False):
    """S = 3, N = 3, stride max_len + 2.  Stream 0: an empty hypothesis, one of exactly max_len tokens, one with a token >= K (dropped).
    Stream 1, count 2: an entry with NaN logp (dropped), a plain one, and a slot beyond the count.  Stream 2: a plain entry, the same
    tokens with the same logp (equal z: the tie goes to the lower q), and a plain one -- entry 8, alone in its group at E = 4.
    more_streams: S = 5, stream 3 with a count of 0 and stream 4 with a count of N + 2 (rejected).  Every token behind an entry's
    length and every slot that may not be read carries `poison` (tokens), -7 (lengths) and NaN (logp).
    -> hyp, hyp_len, count, logp, errors"""
    rng = np.random.RandomState(seed)
    S, N, stride = (5 if more_streams else 3), 3, max_len + 2
    hyp = np.full((S, N, stride), poison, np.int32)
    hyp_len = np.full((S, N), -7, np.int32)
    logp = np.full((S, N), np.nan, F32)
    same = rng.randint(1, K, size=5).tolist()
    rows = {(0, 0): [], (0, 1): rng.randint(1, K, size=max_len).tolist(), (0, 2): [1, K, 2], (1, 0): rng.randint(1, K, size=4).tolist(),
            (1, 1): rng.randint(1, K, size=3).tolist(), (2, 0): same, (2, 1): same, (2, 2): rng.randint(1, K, size=6).tolist()}
    for (s, q), h in rows.items():
        hyp[s, q, :len(h)], hyp_len[s, q], logp[s, q] = h, len(h), -1.0 - 0.5 * q - 0.25 * s
    logp[1, 0] = np.nan
    logp[2, 1] = logp[2, 0]
    count = np.array([3, 2, 3, 0, N + 2][:S], np.int32)
    errors = rng.randint(0, 5, size=(S, N)).astype(np.int32)
    return hyp, hyp_len, count, logp, errors
