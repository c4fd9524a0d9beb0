"""The numpy twin of klstm_ctc_beam_decode_lm (include/klstm.h; tests/test_ctc_beam_lm.py, tests/test_ctc_beam_lm_gpu.py), host only: the
search of tests/ctc_beam_ref.py with a label language model fused in.  The LM is a dense deterministic weighted automaton over the
labels: state 0 is the start, label c leads from state q to next[q][c] and multiplies the prefix probability by weight[q][c];
final[q] (optional) multiplies a hypothesis that ends in q.  The twin IS the definition.  The frame, the list rule and the accounting
are the ones of tests/ctc_beam_ref.py (frame, nbest_list, errors_and_totals), given the tables; what they do with them:
  state            every prefix-tree node carries an LM state: 0 for the empty prefix, next[state_i][c] for entry i extended by c
  fused emission   f = flush(float32(e[c] * flush(weight[state_i][c]))), flush being the emission rule (NaN or below 2^-60: exactly 0,
                   above 2^60: 2^60); f = 0 where next[state_i][c] lies outside [0, Q).  The extension's value is float32(p * f), p
                   being pb or pb + pnb as without an LM, both where it is merged into the stay entry of the same prefix and where
                   it becomes a list entry.  e * g first, then the product with p: every product stays inside [2^-120, 2^121].
                   Candidates are chosen by the emission alone; stay entries, selection, ties and rescale do not know of the LM
  final weights    tf = float32(total * flush(final[state])); the list is the entries with tf > 0 by tf descending (ties: the earlier
                   beam position), the first N; none: the first beam entry alone with score -inf.  Without `final` the list is
                   beam_twin's.  The blank column of both tables is never read.
  score            the FUSED score, acoustic times LM as the search summed them: float(log(double(tf)) + E ln 2)
  textbook_lm64()  the yardstick: textbook64 with the same factor on every extension, float64, all K - 1 classes
  lm_logw64()      the sum of the log weights along a labelling (+ log final): what the LM adds to label_logp64"""
import math

import numpy as np

from tests.ctc_beam_ref import Stream, beam_totals, emissions, emissions64, errors_and_totals, frame, nbest_list


def lm_tables(lm):
    """(next, weight, final or None) -> (int64 [Q, K], flushed float32 [Q, K], flushed float32 [Q] or None)"""
    nxt, wt, fin = lm
    nxt = np.asarray(nxt).astype(np.int64)
    wt = emissions(np.asarray(wt, np.float32))
    assert nxt.ndim == 2 and nxt.shape == wt.shape
    return nxt, wt, (emissions(np.asarray(fin, np.float32)) if fin is not None else None)


def beam_stream_lm(e, blank, B, C, nxt_tab, wt_tab, stats=None):
    """e [n, K] emissions of the valid frames; nxt_tab, wt_tab of lm_tables().  -> (entries, E): entries in beam order, each (prefix
    list, pb, pnb, LM state) after the last rescale.  stats: a dict whose "merges" counts the extensions with f > 0 that went into a
    stay entry."""
    z = Stream()
    for row in e:
        frame(z, row, blank, B, C, nxt_tab, wt_tab, stats)
    return [(z.prefix(nd), pb, pnb, z.st[nd]) for nd, pb, pnb in z.beam], z.E


def beam_twin_lm(y, lens, blank, beam, cands, nbest, lm, w=None, refs=None, stats=None):
    """beam_twin of tests/ctc_beam_ref.py with lm = (next [Q, K], weight [Q, K], final [Q] or None); the same dict, and "state": the
    LM state of every listed hypothesis"""
    y = np.asarray(y, dtype=np.float32)
    T, S, K = y.shape
    nxt_tab, wt_tab, fin = lm_tables(lm)
    assert nxt_tab.shape[1] == K
    hyp, score, count, state = [], [], [], []
    for s in range(S):
        n = lens[s]
        if not 0 < n <= T:
            hyp.append([]); score.append([]); count.append(0); state.append([])
            continue
        ent, E = beam_stream_lm(emissions(y[:n, s], w), blank, beam, cands, nxt_tab, wt_tab, stats)
        live, sc = nbest_list(beam_totals(ent), E, nbest, None if fin is None else [fin[q] for _, _, _, q in ent])
        hyp.append([ent[i][0] for i in live]); score.append(sc); count.append(len(live))
        state.append([ent[i][3] for i in live])
    errors, totals = errors_and_totals(hyp, count, lens, T, K, blank, nbest, refs)
    return dict(hyp=hyp, score=score, nbest_count=count, errors=errors, totals=totals, state=state)


def lm_walk(nxt_tab, labels):
    """the LM state after `labels`, or -1 where a transition leaves [0, Q)"""
    q = 0
    for c in labels:
        q = int(nxt_tab[q, int(c)])
        if not 0 <= q < nxt_tab.shape[0]:
            return -1
    return q


def lm_logw64(lm, labels, with_final=True):
    """sum of log weight along labels (+ log final of the state reached), float64; -inf where a factor is 0 or a transition is bad"""
    nxt_tab, wt_tab, fin = lm
    nxt_tab = np.asarray(nxt_tab).astype(np.int64)
    wt = emissions64(np.asarray(wt_tab, np.float32))
    q, acc = 0, 0.0
    for c in labels:
        q1 = int(nxt_tab[q, int(c)])
        g = wt[q, int(c)]
        if not 0 <= q1 < nxt_tab.shape[0] or g <= 0:
            return -math.inf
        acc += math.log(g)
        q = q1
    if with_final and fin is not None:
        g = emissions64(np.asarray(fin, np.float32))[q]
        if g <= 0:
            return -math.inf
        acc += math.log(g)
    return acc


def textbook_lm64(e, blank, B, lm):
    """e [n, K] float64.  -> [(prefix tuple, log p)] best first: textbook64 of tests/ctc_beam_ref.py with the factor weight[state][c] on
    every extension (0 where next leaves [0, Q)) and final[state] on every hypothesis at the end, float64, every class an extension"""
    nxt_tab, wt_tab, fin = lm
    nxt_tab = np.asarray(nxt_tab).astype(np.int64)
    wt = emissions64(np.asarray(wt_tab, np.float32))
    Q, K = nxt_tab.shape
    beam = {(): (1.0, 0.0)}
    state = {(): 0}
    logscale = 0.0
    for t in range(e.shape[0]):
        row = e[t]
        nxt = {}

        def add(p, b, nb):
            ob, onb = nxt.get(p, (0.0, 0.0))
            nxt[p] = (ob + b, onb + nb)
        for p, (pb, pnb) in beam.items():
            add(p, (pb + pnb) * row[blank], pnb * row[p[-1]] if p else 0.0)
            q = state[p]
            for c in range(K):
                if c == blank:
                    continue
                q1 = int(nxt_tab[q, c])
                if not 0 <= q1 < Q:
                    continue
                state[p + (c,)] = q1
                add(p + (c,), 0.0, (pb if p and p[-1] == c else pb + pnb) * (row[c] * wt[q, c]))
        best = sorted(nxt.items(), key=lambda it: (-(it[1][0] + it[1][1]), it[0]))[:B]
        m = best[0][1][0] + best[0][1][1]
        if m > 0:
            logscale += math.log(m)
            best = [(p, (b / m, nb / m)) for p, (b, nb) in best]
        beam = dict(best)
        state = {p: state[p] for p in beam}
    f64 = emissions64(np.asarray(fin, np.float32)) if fin is not None else None
    out = []
    for p, (b, nb) in beam.items():
        tot = (b + nb) * (f64[state[p]] if f64 is not None else 1.0)
        out.append((p, (math.log(tot) + logscale) if tot > 0 else -math.inf))
    return sorted(out, key=lambda it: (-it[1], it[0]))
