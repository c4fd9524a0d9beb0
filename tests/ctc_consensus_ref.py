"""The numpy twin of klstm_ctc_consensus (include/klstm.h; kaldi-lstm_amd/csrc/klstm_ctc_consensus.hip), host only: MBR
decoding and unit confidences over n-best lists, every sum in the order the device takes it, in float64.  consensus() is the twin;
brute() is an independent brute force (full tables in Python ints, math.fsum) that tests/test_ctc_consensus.py holds the twin against.
make_lists() is the generator of the GPU tests' inputs."""
import math

import numpy as np

from tests.nbest_ref import H0, HMUL, M64, beam_hash, levenshtein, split_words, word_key  # noqa: F401  (for the tests)

TOTALS = 10


def units_of(tokens, separator):
    """the unit keys of a token list: the tokens, or the keys of its words (maximal runs of tokens other than the separator)"""
    if separator < 0:
        return [int(t) for t in tokens]
    return [word_key(w) for w in split_words(tokens, separator)]


def table(a, b):
    D = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) + 1):
        D[i][0] = i
    for j in range(len(b) + 1):
        D[0][j] = j
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            D[i][j] = min(D[i - 1][j] + 1, D[i][j - 1] + 1, D[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
    return D


def table_rows(a, b):
    """table(a, b) as an int64 array, row by row in the device's row formulation (brute() keeps to the plain table)"""
    cols = np.asarray(b, dtype=np.uint64)
    j = np.arange(len(b) + 1)
    D = np.empty((len(a) + 1, len(b) + 1), np.int64)
    D[0] = j
    for i, tok in enumerate(a, 1):
        tmp = np.empty(len(b) + 1, np.int64)
        tmp[0] = i
        tmp[1:] = np.minimum(D[i - 1, 1:] + 1, D[i - 1, :-1] + (cols != np.uint64(tok)))
        D[i] = j + np.minimum.accumulate(tmp - j)
    return D


def matched(a, b):
    """THE alignment of the pivot a against b: [slot i of a is left by a diagonal step with equal units], the fixed walk"""
    D = table_rows(a, b)
    i, j = len(a), len(b)
    out = [False] * len(a)
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i][j] == D[i - 1][j - 1] + (a[i - 1] != b[j - 1]):
            out[i - 1] = a[i - 1] == b[j - 1]
            i, j = i - 1, j - 1
        elif i > 0 and D[i][j] == D[i - 1][j] + 1:
            i -= 1
        else:
            j -= 1
    return out


def live_entries(hyp, hyp_len, count, logp, max_len):
    """per stream (status: 'done' / 'idle' / 'rejected', the live q's, entries dropped); slots q >= count are not read"""
    S, N, stride = hyp.shape
    out = []
    for s in range(S):
        c = int(count[s])
        if c < 0 or c > N:
            out.append(("rejected", [], 0))
            continue
        live = [q for q in range(c) if np.isfinite(logp[s, q]) and 0 <= hyp_len[s, q] <= min(stride, max_len)
                and not (hyp[s, q, :hyp_len[s, q]] < 0).any()]
        out.append(("done" if live else "idle", live, c - len(live)))
    return out


def consensus(hyp, hyp_len, count, logp, scale=1.0, separator=-1, pivot_mode=1, errors=None, max_len=None):
    """-> dict of numpy arrays named as the C entry names them, plus totals [10] (what ONE call adds) and conf_len [S]"""
    hyp, hyp_len, count = np.asarray(hyp), np.asarray(hyp_len), np.asarray(count)
    logp = np.asarray(logp, dtype=np.float32)
    S, N, stride = hyp.shape
    max_len = min(1023, stride) if max_len is None else max_len
    sc = np.float64(np.float32(scale))
    o = dict(pick=np.full(S, -1, np.int32), map=np.full(S, -1, np.int32), mbr=np.full(S, -1, np.int32), post=np.zeros((S, N), np.float32),
             risk=np.full((S, N), -1, np.float32), unit_len=np.zeros((S, N), np.int32), conf=np.zeros((S, stride), np.float32),
             dist=np.full((S, N, N), -1, np.int32), conf_len=np.zeros(S, np.int32), risk64=np.full((S, N), -1.0), post64=np.zeros((S, N)),
             conf64=np.zeros((S, stride)), z64=np.full((S, N), np.nan))
    tot = np.zeros(TOTALS)
    for s, (status, live, dropped) in enumerate(live_entries(hyp, hyp_len, count, logp, max_len)):
        units = {q: units_of(hyp[s, q, :hyp_len[s, q]].tolist(), separator) for q in live}
        for q in live:
            o["unit_len"][s, q] = len(units[q])
        for q in live:
            for r in live:
                if r >= q:
                    o["dist"][s, q, r] = o["dist"][s, r, q] = levenshtein(units[q], units[r]) if r > q else 0
        tot[7] += dropped
        if status != "done":
            tot[1] += 1
            continue
        z = {q: sc * np.float64(logp[s, q]) for q in live}
        for q in live:
            o["z64"][s, q] = z[q]
        m = max(z.values())
        e = {q: np.exp(z[q] - m) for q in live}
        Z = np.float64(0.0)
        for q in live:
            Z = Z + e[q]
        P = {q: e[q] / Z for q in live}
        R = {}
        for q in live:
            acc = np.float64(0.0)
            for r in live:
                acc = acc + P[r] * np.float64(o["dist"][s, q, r])
            R[q] = acc
        imap = imbr = live[0]
        for q in live:
            if z[q] > z[imap]:
                imap = q
            if R[q] < R[imbr]:
                imbr = q
        pick = imbr if pivot_mode else imap
        for q in live:
            o["post"][s, q], o["risk"][s, q], o["post64"][s, q], o["risk64"][s, q] = P[q], R[q], P[q], R[q]
        o["pick"][s], o["map"][s], o["mbr"][s] = pick, imap, imbr
        m_r = {r: matched(units[pick], units[r]) for r in live}
        csum = np.float64(0.0)
        for u in range(len(units[pick])):
            c = np.float64(0.0)
            for r in live:
                if m_r[r][u]:
                    c = c + P[r]
            o["conf"][s, u], o["conf64"][s, u] = c, c
            csum = csum + c
        o["conf_len"][s] = len(units[pick])
        tot[0] += 1
        tot[2] += R[pick]
        tot[3] += R[imap]
        tot[4] += imbr != imap
        tot[5] += len(units[pick])
        tot[6] += csum
        if errors is not None:
            tot[8] += int(errors[s, pick])
            tot[9] += int(errors[s, imap])
    o["totals"] = tot
    return o


def brute(lists, logps, scale, separator, pivot_mode):
    """ONE stream of live entries, independently: full tables in Python ints, math.fsum for every sum -> dict(dist, post, risk, map, mbr,
    pick, conf)"""
    units = []
    for toks in lists:
        if separator < 0:
            units.append(list(toks))
        else:                                  # words as tuples of tokens: no hash
            words, cur = [], []
            for t in toks:
                if t == separator:
                    if cur:
                        words.append(tuple(cur))
                    cur = []
                else:
                    cur.append(t)
            if cur:
                words.append(tuple(cur))
            units.append(words)
    n = len(lists)
    dist = [[table(units[q], units[r])[-1][-1] for r in range(n)] for q in range(n)]
    z = [float(np.float32(scale)) * float(np.float32(l)) for l in logps]
    m = max(z)
    e = [math.exp(v - m) for v in z]
    Z = math.fsum(e)
    post = [v / Z for v in e]
    risk = [math.fsum(post[r] * dist[q][r] for r in range(n)) for q in range(n)]
    imap = max(range(n), key=lambda q: (z[q], -q))
    imbr = min(range(n), key=lambda q: (risk[q], q))
    pick = imbr if pivot_mode else imap
    conf = []
    for u in range(len(units[pick])):
        terms = []
        for r in range(n):
            # the fixed walk, written out again on the full table
            a, b = units[pick], units[r]
            D = table(a, b)
            i, j, hit = len(a), len(b), False
            while i > 0:
                if j > 0 and D[i][j] == D[i - 1][j - 1] + (a[i - 1] != b[j - 1]):
                    if i - 1 == u:
                        hit = a[i - 1] == b[j - 1]
                    i, j = i - 1, j - 1
                elif D[i][j] == D[i - 1][j] + 1:
                    i -= 1
                else:
                    j -= 1
            if hit:
                terms.append(post[r])
        conf.append(math.fsum(terms))
    return dict(dist=dist, post=post, risk=risk, map=imap, mbr=imbr, pick=pick, conf=conf)


def make_lists(seed, S, N, L, K=40, spread=4.0, stride=None, lens=None):
    """the GPU tests' lists: per stream one base sequence of L (or lens[s]) tokens in [1, K), every entry 0-3 random substitutions,
    deletions or insertions of it; logp sorted draws of -spread * U(0, 1), best first.  -> hyp [S, N, stride], hyp_len, count, logp"""
    rng = np.random.default_rng(seed)
    rows = []
    for s in range(S):
        base = rng.integers(1, K, size=L if lens is None else lens[s]).tolist()
        ent = []
        for q in range(N):
            for _ in range(1000):              # the entries of a list are distinct, as the search's are
                h = list(base)
                for _ in range(int(rng.integers(0, 4))):
                    kind, pos = int(rng.integers(0, 3)), int(rng.integers(0, len(h) + 1))
                    if kind == 0 and h:
                        h[min(pos, len(h) - 1)] = int(rng.integers(1, K))
                    elif kind == 1 and h:
                        del h[min(pos, len(h) - 1)]
                    elif kind == 2:
                        h.insert(pos, int(rng.integers(1, K)))
                if h not in ent:
                    break
            assert h not in ent, "the shape leaves no room for N distinct entries"
            ent.append(h)
        rows.append(ent)
    longest = max(len(h) for ent in rows for h in ent)
    stride = max(longest, 1) if stride is None else stride
    hyp = np.zeros((S, N, stride), np.int32)
    hyp_len = np.zeros((S, N), np.int32)
    for s, ent in enumerate(rows):
        for q, h in enumerate(ent):
            hyp[s, q, :len(h)] = h
            hyp_len[s, q] = len(h)
    logp = -np.sort(spread * rng.random((S, N)), axis=1).astype(np.float32)
    return hyp, hyp_len, np.full(S, N, np.int32), logp


def gaps(o):
    """(the smallest relative gap between the two smallest risks, between the two largest z) over the done streams with
    at least two live entries"""
    g_r, g_p = np.inf, np.inf
    for s in range(len(o["pick"])):
        if o["pick"][s] < 0:
            continue
        live = np.flatnonzero(o["risk64"][s] >= 0)
        if len(live) < 2:
            continue
        r = np.sort(o["risk64"][s, live])
        g_r = min(g_r, (r[1] - r[0]) / max(r[1], 1e-300))
        p = np.sort(o["z64"][s, live])[::-1]
        g_p = min(g_p, (p[0] - p[1]) / max(abs(p[0]), abs(p[1]), 1e-300))
    return g_r, g_p
