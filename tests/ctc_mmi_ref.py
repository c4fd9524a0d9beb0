"""Yardsticks of the MMI (CTC-CRF) tests (tests/test_ctc_mmi.py, tests/test_ctc_mmi_gpu.py; klstm_ctc_mmi_eval of include/klstm.h), host only.
A language model is the tuple (next int [Q, K], weight float32 [Q, K], final float32 [Q] or None) that kaldi_lstm_amd.lm builds.
  present()        which arcs exist: k != blank, weight > 0 (a NaN is not), next inside [0, Q)
  lm_logw()        log W(labels): the walk over the automaton in float64, -inf where an arc is absent or the final weight is not > 0
  statuses()       idle / rejected / counted from the lengths, the labels and the model alone
  enumerate_z()    Z and W-weighted path sums by brute force over all K^T frame paths (tiny cases)
  truth64()        the recursion of the issue over the dense (q, c) states in float64, linear domain, every frame's row scaled by a power
                   of two whose exponents are summed as integers.  "R(q) - alpha(q, k)" is summed WITHOUT the excluded term (a product
                   with 1 - I): the same recursion, but no cancellation can touch the yardstick where posteriors are clamped zeros
  plain32()        the same recursion in numpy float32 in the log domain (np.logaddexp, no rescaling): what a straightforward fp32
                   implementation delivers; the bar of the device is 4 x its error
  objective64()    loss of ONE stream as a function of float64 posteriors: what the gradient is pinned against by central differences"""
import itertools

import numpy as np

FLT_MIN = float(np.finfo(np.float32).tiny)


def present(lm, blank):
    nxt, w = np.asarray(lm[0]), np.asarray(lm[1], dtype=np.float32)
    Q, K = nxt.shape
    with np.errstate(invalid="ignore"):
        p = (w > 0) & (nxt >= 0) & (nxt < Q)
    p[:, blank] = False
    return p


def _final(lm):
    Q = np.asarray(lm[0]).shape[0]
    if lm[2] is None:
        return np.ones(Q)
    f = np.asarray(lm[2], dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(f > 0, f, 0.0)


def lm_logw(lm, blank, labels):
    p, nxt, w, fin = present(lm, blank), np.asarray(lm[0]), np.asarray(lm[1], dtype=np.float32).astype(np.float64), _final(lm)
    q, lw = 0, 0.0
    for c in labels:
        if not (0 <= c < nxt.shape[1]) or not p[q, c]:
            return -np.inf
        lw += np.log(w[q, c])
        q = int(nxt[q, c])
    return lw + np.log(fin[q]) if fin[q] > 0 else -np.inf


def statuses(lens, labels, lm, K, blank, T):
    out = []
    for n, lab in zip(lens, labels):
        lab = list(lab)
        rep = sum(1 for a, b in zip(lab[:-1], lab[1:]) if a == b)
        bad = any(c < 0 or c >= K or c == blank for c in lab)
        if n == 0:
            out.append("idle")
        elif n < 0 or n > T or bad or n < len(lab) + rep or len(lab) > 1023 or lm_logw(lm, blank, lab) == -np.inf:
            out.append("rejected")
        else:
            out.append("counted")
    return out


def enumerate_z(y, lm, blank, labels=None):
    """y [T, K] float64.  sum over all K^T paths of W(collapse(path)) prod_t y; with labels: only the paths that collapse to them, W left out"""
    T, K = y.shape
    tot = 0.0
    for path in itertools.product(range(K), repeat=T):
        col = [k for k in (k for k, _ in itertools.groupby(path)) if k != blank]
        pr = float(np.prod([y[t, path[t]] for t in range(T)]))
        if labels is None:
            lw = lm_logw(lm, blank, col)
            tot += np.exp(lw) * pr if lw > -np.inf else 0.0
        elif col == list(labels):
            tot += pr
    return tot


def _ctc_fb(ly, lab, blank):
    """log-domain forward-backward over the CTC lattice of `lab` in the dtype of ly [n, K] (log posteriors) -> (log p, gamma [n, K])"""
    dt = ly.dtype
    n, K = ly.shape
    L = len(lab)
    N = 2 * L + 1
    ext = np.full(N, blank, dtype=np.int64)
    ext[1::2] = lab
    skip = np.zeros(N, dtype=bool)
    skip[3::2] = np.asarray(lab[1:]) != np.asarray(lab[:-1])
    skip_b = np.concatenate([skip[2:], [False, False]])[:N]
    em = ly[:, ext]
    ninf = np.full(2, -np.inf, dt)
    A = np.full((n, N), -np.inf, dt)
    B = np.full((n, N), -np.inf, dt)
    A[0, :2] = em[0, :2]
    B[n - 1, max(N - 2, 0):] = 0.0
    with np.errstate(invalid="ignore"):
        for t in range(1, n):
            p = np.concatenate([ninf, A[t - 1]])
            A[t] = np.logaddexp(np.logaddexp(p[2:], p[1:-1]), np.where(skip, p[:-2], -np.inf).astype(dt)) + em[t]
        for t in range(n - 2, -1, -1):
            p = np.concatenate([B[t + 1] + em[t + 1], ninf])
            B[t] = np.logaddexp(np.logaddexp(p[:-2], p[1:-1]), np.where(skip_b, p[2:], -np.inf).astype(dt))
        logp = np.logaddexp.reduce(A[n - 1, max(N - 2, 0):])
        g = A + B
        m = g.max(1, keepdims=True)
        g = g - (m + np.log(np.exp(g - m).sum(1, keepdims=True, dtype=dt)))
    gam = np.zeros((n, K), dt)
    np.add.at(gam, (np.arange(n)[:, None], ext[None, :]), np.exp(g))
    return logp, gam


def _den_lin64(yc, lm, blank):
    """yc [n, K] float64, clamped.  -> (log Z, gamma_den [n, K]) by the scaled linear recursion over the dense (q, c) states"""
    p, nxt, fin = present(lm, blank), np.asarray(lm[0]), _final(lm)
    w = np.where(p, np.asarray(lm[1], dtype=np.float32).astype(np.float64), 0.0)
    Q, K = nxt.shape
    n = yc.shape[0]
    off = 1.0 - np.eye(K)
    qs, ks = np.nonzero(p)
    dst = nxt[qs, ks]
    lab = np.arange(K) != blank
    al = np.zeros((n, Q, K))
    be = np.zeros((n, Q, K))
    a = np.zeros((Q, K))
    a[0, blank] = 1.0
    esum = 0

    def scaled(row):
        m = row.max()
        e = int(np.floor(np.log2(m))) if m > 0 and np.isfinite(m) else 0
        return np.ldexp(row, -e), e
    for t in range(n):
        excl = a @ off                                  # excl[q, k] = sum over c != k of a[q, c]
        new = np.zeros((Q, K))
        new[:, blank] = yc[t, blank] * (excl[:, blank] + a[:, blank])
        inc = np.zeros((Q, K))
        np.add.at(inc, (dst, ks), w[qs, ks] * excl[qs, ks])
        new[:, lab] = (yc[t][None, :] * (a + inc))[:, lab]
        a, e = scaled(new)
        esum += e
        al[t] = a
    logz = np.log((a * fin[:, None]).sum()) + esum * np.log(2.0)
    b = np.repeat(fin[:, None], K, 1)
    b, _ = scaled(b)
    be[n - 1] = b
    for t in range(n - 2, -1, -1):
        y1 = yc[t + 1]
        G = np.zeros((Q, K))
        G[qs, ks] = w[qs, ks] * y1[ks] * b[dst, ks]
        new = (y1[blank] * b[:, blank])[:, None] + G @ off
        new[:, lab] += (y1[None, :] * b)[:, lab]
        b, _ = scaled(new)
        be[t] = b
    g = (al * be).sum(1)
    return logz, g / g.sum(1, keepdims=True)


def _den_log32(ly, lm, blank):
    """ly [n, K] float32 log posteriors.  The same recursion, log domain, float32 throughout, no scaling"""
    f32 = np.float32
    p, nxt = present(lm, blank), np.asarray(lm[0])
    Q, K = nxt.shape
    n = ly.shape[0]
    with np.errstate(divide="ignore"):
        lw = np.where(p, np.log(np.where(p, np.asarray(lm[1], dtype=f32), f32(1))), f32(-np.inf)).astype(f32)
        lfin = np.log(_final(lm).astype(f32)).astype(f32)
    diag = np.where(np.eye(K, dtype=bool), f32(-np.inf), f32(0))[None]        # [1, K, K]: added to a[q, None, c], -inf where c == k
    qs, ks = np.nonzero(p)
    dst = nxt[qs, ks]
    lab = np.arange(K) != blank
    al = np.full((n, Q, K), -np.inf, f32)
    be = np.full((n, Q, K), -np.inf, f32)
    a = np.full((Q, K), -np.inf, f32)
    a[0, blank] = 0
    with np.errstate(invalid="ignore"):
        for t in range(n):
            excl = np.logaddexp.reduce(a[:, None, :] + diag, axis=-1)
            new = np.full((Q, K), -np.inf, f32)
            new[:, blank] = ly[t, blank] + np.logaddexp(excl[:, blank], a[:, blank])
            inc = a.copy()
            np.logaddexp.at(inc, (dst, ks), lw[qs, ks] + excl[qs, ks])
            new[:, lab] = (ly[t][None, :] + inc)[:, lab]
            a = new.astype(f32)
            al[t] = a
        logz = np.logaddexp.reduce((a + lfin[:, None]).ravel())
        b = np.repeat(lfin[:, None], K, 1).astype(f32)
        be[n - 1] = b
        for t in range(n - 2, -1, -1):
            y1 = ly[t + 1]
            G = np.full((Q, K), -np.inf, f32)
            G[qs, ks] = lw[qs, ks] + y1[ks] + b[dst, ks]
            new = np.logaddexp((y1[blank] + b[:, blank])[:, None], np.logaddexp.reduce(G[:, None, :] + diag, axis=-1))
            new[:, lab] = np.logaddexp(new, y1[None, :] + b)[:, lab]
            b = new.astype(f32)
            be[t] = b
        g = np.logaddexp.reduce(al + be, axis=1)                              # [n, K]
        g = g - np.logaddexp.reduce(g, axis=1, keepdims=True)
    return f32(logz), np.exp(g).astype(f32)


def objective64(y, lab, lm, blank, lam=0.0):
    """y [n, K] float64 posteriors of one counted stream -> dict(loss, num_logp, logz, logw, gamma_den, gamma_ref)"""
    yc = np.maximum(np.where(np.isnan(y), FLT_MIN, y), FLT_MIN)
    logp, gref = _ctc_fb(np.log(yc), list(lab), blank)
    logz, gden = _den_lin64(yc, lm, blank)
    logw = lm_logw(lm, blank, lab)
    return dict(loss=-logp - logw + logz, num_logp=logp, logz=logz, logw=logw, gamma_den=gden, gamma_ref=gref)


def truth64(y, lens, labels, lm, blank, lam=0.0):
    """y [T, S, K] float32.  -> dict(loss [S], diff [T, S, K], num_logp, logz, logw [S], status) in float64; idle: loss 0, rejected: +inf,
    both with zero rows, as are the padding rows"""
    y = np.asarray(y, dtype=np.float32)
    T, S, K = y.shape
    st = statuses(lens, labels, lm, K, blank, T)
    out = dict(loss=np.zeros(S), diff=np.zeros((T, S, K)), num_logp=np.zeros(S), logz=np.zeros(S), logw=np.zeros(S), status=st)
    for s in range(S):
        if st[s] == "rejected":
            out["loss"][s] = np.inf
        if st[s] != "counted":
            continue
        n = lens[s]
        yd = y[:n, s].astype(np.float64)
        o = objective64(yd, labels[s], lm, blank)
        out["loss"][s], out["num_logp"][s], out["logz"][s], out["logw"][s] = o["loss"], o["num_logp"], o["logz"], o["logw"]
        out["diff"][:n, s] = o["gamma_den"] - o["gamma_ref"] + lam * (yd - o["gamma_ref"])
    return out


def plain32(y, lens, labels, lm, blank, lam=0.0, status=None):
    """the float32 log-domain twin of truth64 -> (loss [S] float32, diff [T, S, K] float32)"""
    f32 = np.float32
    y = np.asarray(y, dtype=f32)
    T, S, K = y.shape
    st = status or statuses(lens, labels, lm, K, blank, T)
    loss, diff = np.zeros(S, f32), np.zeros((T, S, K), f32)
    for s in range(S):
        if st[s] == "rejected":
            loss[s] = np.inf
        if st[s] != "counted":
            continue
        n = lens[s]
        ys = y[:n, s]
        ly = np.log(np.maximum(np.where(np.isnan(ys), f32(FLT_MIN), ys), f32(FLT_MIN))).astype(f32)
        logp, gref = _ctc_fb(ly, list(labels[s]), blank)
        logz, gden = _den_log32(ly, lm, blank)
        loss[s] = f32(-logp) - f32(lm_logw(lm, blank, labels[s])) + logz
        diff[:n, s] = gden - gref + f32(lam) * (ys - gref)
    return loss, diff


def pooled_errors(loss, diff, t64, lens):
    """(max |diff - truth| over the valid rows, max |loss - truth| / max(1, |truth|)) pooled over the counted streams"""
    e = r = 0.0
    for s, n in enumerate(lens):
        if t64["status"][s] == "counted":
            e = max(e, float(np.abs(np.asarray(diff[:n, s], dtype=np.float64) - t64["diff"][:n, s]).max()))
            r = max(r, abs(float(loss[s]) - t64["loss"][s]) / max(1.0, abs(t64["loss"][s])))
    return e, r


def all_ones_lm(K):
    """Q = 1, every label weight 1, final 1: Z = 1, gamma_den = y, the loss is the CTC loss"""
    return np.zeros((1, K), np.int32), np.ones((1, K), np.float32), np.ones(1, np.float32)


def make_lm(kind, K, blank, seed=0):
    """the language models of the grid: unigram / bigram / trigram add-k models estimated from seeded random sequences, and a lexicon trie
    (forbidden arcs with next -1, a final vector with zeros) over the first non-blank classes with the last one as the separator"""
    from importlib import import_module
    lm = import_module("kaldi_lstm_amd").lm if hasattr(import_module("kaldi_lstm_amd"), "lm") else import_module("kaldi_lstm_amd.lm")
    rng = np.random.RandomState(100 + seed)
    classes = [c for c in range(K) if c != blank]
    if kind == "lexicon":
        sep, letters = classes[-1], classes[:-1]
        words = [[letters[0]], [letters[0], letters[-1]], [letters[-1], letters[-1], letters[0]]]
        return lm.lexicon_label_lm(words, K, blank, sep)
    order = {"unigram": 1, "bigram": 2, "trigram": 3}[kind]
    seqs = [[classes[i] for i in rng.randint(0, len(classes), rng.randint(1, 6))] for _ in range(12)]
    return lm.ngram_label_lm(seqs, K, blank, order=order, add_k=0.5)
