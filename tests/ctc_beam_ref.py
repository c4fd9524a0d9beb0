"""The numpy twin of klstm_ctc_beam_decode (include/klstm.h; tests/test_ctc_beam.py, tests/test_ctc_beam_gpu.py), host only.  The twin IS
the definition: CTC prefix beam search in the LINEAR domain, every step one float32 operation rounded to nearest (a product or a sum,
never a fused one), an exact power-of-two rescale per frame, prefix identity by (length, 64-bit hash).  Every integer the kernel
produces must equal the twin exactly, and so must the bits of every probability; only the final double log can differ by an ulp.
  emissions()      e[k] = float32(y[k] * w[k]) (y[k] without weights); NaN or below 2^-60 counts as exactly 0, above 2^60 (+inf too)
                   as 2^60: every product then stays inside [2^-120, 2^121], no denormal, no overflow, no NaN on the chain
  candidates()     the non-blank classes with the C largest e, larger value first, then the lower column; only e > 0 counts
  frame()          ONE frame on a Stream state: stay entries, extensions (merged into the stay entry of the same prefix where the
                   beam holds it), selection of the B largest totals (ties: earlier list position), rescale.  The only frame there
                   is: the twins with a language model (tests/ctc_beam_lm_ref.py) and fed chunk by chunk
                   (tests/ctc_beam_stream_ref.py) run it too, so a search resumed at any frame boundary has the same bits
  beam_stream()    the frame chain of one utterance
  nbest_list()     the list rule of all the twins: the first N beam entries with a total > 0 (with final weights: by tf); a DEAD
                   utterance (len > 0 and every total 0: a frame without any emission) lists its first beam entry alone with
                   score -inf
  errors_and_totals()  the accounting of all the twins against the references
  beam_twin()      everything klstm_ctc_beam_decode returns, with the stream statuses of the header
  textbook64()     the yardstick: the textbook prefix beam search keyed by a dictionary of prefixes, float64, all K - 1 classes
  label_logp64()   the exact float64 log p(labels | e) by the CTC forward recurrence (per-frame normalisation, no underflow)"""
import math

import numpy as np

from tests.nbest_ref import H0 as H_EMPTY, beam_hash as hash_step, levenshtein  # noqa: F401  (levenshtein: for the tests)

F = np.float32
TINY = F(2.0 ** -60)
HUGE = F(2.0 ** 60)
LN2 = math.log(2.0)


def prefix_hash(prefix):
    h = H_EMPTY
    for c in prefix:
        h = hash_step(h, int(c))
    return h


def emissions(y, w=None):
    """y [..., K] float32 -> e float32 of the same shape"""
    y = np.asarray(y, dtype=np.float32)
    with np.errstate(all="ignore"):
        v = y if w is None else (y * np.asarray(w, np.float32)).astype(np.float32)
        return np.where(v >= TINY, np.minimum(v, HUGE), F(0)).astype(np.float32)        # NaN >= x is False


def candidates_all(e, blank, C):
    """e [n, K] -> per frame the list of candidate columns (a stable sort of -e over the non-blank columns: ties keep the lower column)"""
    cols = np.delete(np.arange(e.shape[1]), blank)
    v = e[:, cols]
    order = np.argsort(-v, axis=1, kind="stable")[:, :C]
    top = np.take_along_axis(v, order, axis=1)
    return [[int(c) for c, x in zip(cols[o], tv) if x > 0] for o, tv in zip(order, top)]


def candidates(e_row, blank, C):
    return candidates_all(np.asarray(e_row, np.float32)[None, :], blank, C)[0]


class Stream:
    """what the search carries from frame to frame, and what the device holds per stream: the prefix tree (parent, token, length, hash
    and LM state per node), the beam (node, pb, pnb) in beam order, the running exponent E -- the probability of an entry is
    (pb + pnb) * 2^E -- and the frames consumed"""

    def __init__(self):
        self.par, self.tok, self.ln, self.hs, self.st = [-1], [-1], [0], [H_EMPTY], [0]      # node 0: the empty prefix, LM state 0
        self.beam = [(0, F(1), F(0))]
        self.E = 0
        self.frames = 0

    def prefix(self, nd):
        pre = []
        while nd > 0:
            pre.append(self.tok[nd])
            nd = self.par[nd]
        return pre[::-1]


def frame(z, row, blank, B, C, nxt_tab=None, wt_tab=None, stats=None):
    """THE frame of the search, on the stream state z; row: the frame's emissions [K].  Without tables the factor of an extension is
    its emission; with the tables of lm_tables() (tests/ctc_beam_lm_ref.py) it is the fused emission defined there.  stats: a dict
    whose "merges" counts the extensions with a factor > 0 that went into a stay entry."""
    par, tok, ln, hs, st, beam = z.par, z.tok, z.ln, z.hs, z.st, z.beam
    with np.errstate(all="ignore"):
        eb = row[blank]
        cand = candidates(row, blank, C)
        tot = [F(pb + pnb) for _, pb, pnb in beam]
        spb = [F(tot[i] * eb) for i in range(len(beam))]
        spnb = [F(beam[i][2] * row[tok[beam[i][0]]]) if tok[beam[i][0]] >= 0 else F(0) for i in range(len(beam))]
        index = {(ln[nd], hs[nd]): j for j, (nd, _, _) in enumerate(beam)}
        new = []
        for i, (nd, pb, pnb) in enumerate(beam):
            for c in cand:
                if nxt_tab is None:
                    q1, f = 0, row[c]
                else:
                    q1 = int(nxt_tab[st[nd], c])
                    f = F(row[c] * wt_tab[st[nd], c])
                    f = (min(f, HUGE) if f >= TINY else F(0)) if 0 <= q1 < nxt_tab.shape[0] else F(0)
                v = F((pb if c == tok[nd] else tot[i]) * f)
                key = (ln[nd] + 1, hash_step(hs[nd], c))
                j = index.get(key)
                if j is not None:
                    spnb[j] = F(spnb[j] + v)
                    if stats is not None and f > 0:
                        stats["merges"] = stats.get("merges", 0) + 1
                elif v > 0:
                    new.append((nd, c, key, v, q1))
        items = [(F(spb[i] + spnb[i]), i) for i in range(len(beam))] + [(F(F(0) + it[3]), len(beam) + q) for q, it in enumerate(new)]
        items.sort(key=lambda it: -float(it[0]))             # stable: ties keep the list order
        items = items[:B]
        nb = []
        for _, pos in items:
            if pos < len(beam):
                nb.append((beam[pos][0], spb[pos], spnb[pos]))
            else:
                nd, c, key, v, q1 = new[pos - len(beam)]
                par.append(nd); tok.append(c); ln.append(key[0]); hs.append(key[1]); st.append(q1)
                nb.append((len(par) - 1, F(0), v))
        M = items[0][0]
        if M > 0:
            _, k = math.frexp(float(M))
            sc = F(2.0 ** -k)
            z.E += k

            def resc(p):
                p = F(p * sc)
                return p if p >= TINY else F(0)
            nb = [(nd, resc(pb), resc(pnb)) for nd, pb, pnb in nb]
        z.beam = nb
        z.frames += 1


def beam_stream(e, blank, B, C):
    """e [n, K] emissions of the valid frames.  -> (entries, E): entries in beam order, each (prefix list, pb, pnb) after the last
    rescale; E the running exponent: the probability of an entry is (pb + pnb) * 2^E."""
    z = Stream()
    for row in e:
        frame(z, row, blank, B, C)
    return [(z.prefix(nd), pb, pnb) for nd, pb, pnb in z.beam], z.E


def total_score(tf, E):
    with np.errstate(all="ignore"):
        return F(np.log(np.float64(tf)) + E * LN2) if tf > 0 else F(-np.inf)


def nbest_list(tot, E, nbest, fin=None):
    """THE list rule.  tot: the float32 totals pb + pnb of the beam entries, in beam order; fin: the flushed final weight of every
    entry's LM state, or None.  -> (the beam positions listed, their scores): the entries with tf = float32(tot * fin) > 0 (tot
    without fin), in beam order, or by tf descending with fin (ties: the earlier beam position), the first nbest; none: the first
    beam entry alone, DEAD, with score -inf"""
    with np.errstate(all="ignore"):
        tf = list(tot) if fin is None else [F(t * g) for t, g in zip(tot, fin)]
    order = list(range(len(tf)))
    if fin is not None:
        order.sort(key=lambda i: -float(tf[i]))              # stable: ties keep the beam order
    live = [i for i in order if tf[i] > 0][:nbest]
    if not live:
        return [0], [F(-np.inf)]
    return live, [total_score(tf[i], E) for i in live]


def beam_totals(entries):
    """entries (anything, pb, pnb, ...) -> their totals float32(pb + pnb)"""
    with np.errstate(all="ignore"):
        return [F(e[1] + e[2]) for e in entries]


def errors_and_totals(hyp, count, lens, T, K, blank, nbest, refs):
    """THE accounting against the references.  -> (errors [S][N] (-1: not counted), totals [6]: 1-best errors, reference tokens,
    1-best tokens, utterances counted, utterances with a 1-best error, oracle errors), or (None, None) without refs.  A stream counts
    iff it decoded (0 < len <= T) and its reference holds at most 1023 labels, every one a class other than the blank"""
    if refs is None:
        return None, None
    errors, totals = [[-1] * nbest for _ in hyp], [0.0] * 6
    for s in range(len(hyp)):
        r = list(refs[s])
        if not 0 < lens[s] <= T or len(r) > 1023 or any(c < 0 or c >= K or c == blank for c in r):
            continue
        for q, h in enumerate(hyp[s]):
            errors[s][q] = levenshtein(h, r)
        e1 = errors[s][0]
        totals = [totals[0] + e1, totals[1] + len(r), totals[2] + len(hyp[s][0]), totals[3] + 1, totals[4] + (e1 > 0),
                  totals[5] + min(errors[s][:count[s]])]
    return errors, totals


def beam_twin(y, lens, blank, beam, cands, nbest, w=None, refs=None):
    """y [T, S, K] -> dict(hyp: S lists of lists, score: S lists of float32, nbest_count [S], errors [S][N] (-1: not counted) or None,
    totals [6] or None: 1-best errors, reference tokens, 1-best tokens, utterances counted, utterances with a 1-best error, oracle
    errors)"""
    y = np.asarray(y, dtype=np.float32)
    T, S, K = y.shape
    hyp, score, count = [], [], []
    for s in range(S):
        n = lens[s]
        if not 0 < n <= T:
            hyp.append([]); score.append([]); count.append(0)
            continue
        ent, E = beam_stream(emissions(y[:n, s], w), blank, beam, cands)
        live, sc = nbest_list(beam_totals(ent), E, nbest)
        hyp.append([ent[i][0] for i in live]); score.append(sc); count.append(len(live))
    errors, totals = errors_and_totals(hyp, count, lens, T, K, blank, nbest, refs)
    return dict(hyp=hyp, score=score, nbest_count=count, errors=errors, totals=totals)


def emissions64(y, w=None):
    """what the float64 yardsticks read: the twin's emissions without the flush, max(float32(y * w), 0) with NaN as 0 (max(y, 0)
    without weights), capped at 2^60"""
    y = np.asarray(y, dtype=np.float32)
    with np.errstate(all="ignore"):
        v = y if w is None else (y * np.asarray(w, np.float32)).astype(np.float32)
        return np.where(v > 0, np.minimum(v, HUGE), F(0)).astype(np.float64)


def textbook64(e, blank, B):
    """e [n, K] float64.  -> [(prefix tuple, log p)] best first: prefix beam search with a dictionary of prefixes, every class an
    extension, float64, rescaled by the frame's best so nothing underflows"""
    beam = {(): (1.0, 0.0)}
    logscale = 0.0
    K = e.shape[1]
    for t in range(e.shape[0]):
        row = e[t]
        nxt = {}

        def add(p, b, nb):
            ob, onb = nxt.get(p, (0.0, 0.0))
            nxt[p] = (ob + b, onb + nb)
        for p, (pb, pnb) in beam.items():
            add(p, (pb + pnb) * row[blank], pnb * row[p[-1]] if p else 0.0)
            for c in range(K):
                if c == blank:
                    continue
                add(p + (c,), 0.0, (pb if p and p[-1] == c else pb + pnb) * row[c])
        best = sorted(nxt.items(), key=lambda it: (-(it[1][0] + it[1][1]), it[0]))[:B]
        m = best[0][1][0] + best[0][1][1]
        if m > 0:
            logscale += math.log(m)
            best = [(p, (b / m, nb / m)) for p, (b, nb) in best]
        beam = dict(best)
    out = [(p, (math.log(b + nb) + logscale) if b + nb > 0 else -math.inf) for p, (b, nb) in beam.items()]
    return sorted(out, key=lambda it: (-it[1], it[0]))


def label_logp64(e, blank, labels):
    """e [n, K] float64 -> log p(labels | e), exact up to float64 rounding: the forward recurrence over the blank-interleaved labels"""
    ext = [blank]
    for c in labels:
        ext += [int(c), blank]
    U = len(ext)
    ext = np.asarray(ext)
    skip = np.zeros(U, bool)
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    a = np.zeros(U)
    a[0] = 1.0
    logp = 0.0
    for t in range(e.shape[0]):
        if t == 0:
            b = np.zeros(U)
            b[0] = e[0, blank]
            if U > 1:
                b[1] = e[0, ext[1]]
        else:
            b = a.copy()
            b[1:] += a[:-1]
            b[2:] += np.where(skip[2:], a[:-2], 0.0)
            b *= e[t, ext]
        m = b.max()
        if m <= 0:
            return -math.inf
        logp += math.log(m)
        a = b / m
    tail = a[-1] + (a[-2] if U > 1 else 0.0)
    return logp + math.log(tail) if tail > 0 else -math.inf
