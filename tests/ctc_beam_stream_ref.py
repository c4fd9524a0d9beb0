"""The numpy twin of klstm_ctc_beam_stream_step / klstm_ctc_beam_stream_emit (include/klstm.h; tests/test_ctc_beam_stream.py,
tests/test_ctc_beam_stream_gpu.py), host only: the search of tests/ctc_beam_ref.py / tests/ctc_beam_lm_ref.py fed chunk by chunk.  The
twin IS the definition.  Per stream it holds what the device holds: the prefix tree (parent, token, length, hash, LM state per
node), the beam (node, pb, pnb), the exponent E and the frames consumed.
  frame()          ONE frame of beam_stream / beam_stream_lm on that state: the same operations in the same order, so a search resumed
                   at any frame boundary has the bits of the whole-utterance twin
  step()           lens[s] frames of a chunk [T, S, K] per stream; 0 is idle (the state is not touched, even with start set); start[s]
                   begins a new utterance; state that was never started starts at its first non-idle step; a stream whose frames
                   would exceed max_frames is rejected for the call, its state unchanged but for the sticky overflow flag
  emit()           per stream and mode (0 skip, 1 without the final weights, 2 with them) the list beam_twin / beam_twin_lm make of
                   the beam, frames (-1 - frames after an overflow) and stable_len
  stable_len       computed the obvious way: the longest common prefix of the token lists of all beam entries with a total > 0; a
                   DEAD beam: the length of its first entry"""
import math

import numpy as np

from tests.ctc_beam_lm_ref import lm_tables, total_score
from tests.ctc_beam_ref import F, H_EMPTY, HUGE, TINY, candidates, emissions, entry_score, hash_step


class _Stream:
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


def frame(z, row, blank, B, C, nxt_tab=None, wt_tab=None):
    """one frame of beam_stream (nxt_tab None) / beam_stream_lm on the stream state z; row: the frame's emissions [K]"""
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


def common_prefix_len(lists):
    n = min(len(p) for p in lists)
    for d in range(n):
        if any(p[d] != lists[0][d] for p in lists):
            return d
    return n


class BeamStreamTwin:
    def __init__(self, S, K, max_frames, blank, beam, cands, w=None, lm=None):
        self.S, self.K, self.max_frames, self.blank, self.B, self.C, self.w = S, K, max_frames, blank, beam, cands, w
        self.nxt, self.wt, self.fin = lm_tables(lm) if lm is not None else (None, None, None)
        self.z = [None] * S
        self.overflow = [False] * S

    def step(self, chunk, lens, start=None):
        """chunk [T, S, K] float32; rows t >= lens[s] are not read"""
        chunk = np.asarray(chunk, np.float32)
        T = chunk.shape[0]
        for s in range(self.S):
            n = lens[s]
            if not 0 < n <= T:
                continue
            fresh = self.z[s] is None or (start is not None and start[s])
            if (0 if fresh else self.z[s].frames) + n > self.max_frames:
                self.overflow[s] = True
                continue
            if fresh:
                self.z[s] = _Stream()
                self.overflow[s] = False
            e = emissions(chunk[:n, s], self.w)
            for t in range(n):
                frame(self.z[s], e[t], self.blank, self.B, self.C, self.nxt, self.wt)

    def emit(self, mode, nbest):
        """-> dict(hyp: S lists of lists, score: S lists of float32, nbest_count [S], frames [S], stable_len [S] (None where mode 0))"""
        hyp, score, count, frames, stable = [], [], [], [], []
        for s in range(self.S):
            z = self.z[s]
            nfr = z.frames if z is not None else 0
            frames.append(-1 - nfr if self.overflow[s] else nfr)
            if mode[s] not in (1, 2) or z is None:
                hyp.append([]); score.append([]); count.append(0); stable.append(None if mode[s] not in (1, 2) else 0)
                continue
            with np.errstate(all="ignore"):
                tot = [F(pb + pnb) for _, pb, pnb in z.beam]
                fin = self.fin if mode[s] == 2 else None
                tf = tot if fin is None else [F(tot[i] * fin[z.st[nd]]) for i, (nd, _, _) in enumerate(z.beam)]
            order = list(range(len(z.beam)))
            if fin is not None:
                order.sort(key=lambda i: -float(tf[i]))      # stable: ties keep the beam order
            live = [i for i in order if tf[i] > 0][:nbest]
            if live:
                if fin is None:
                    score.append([entry_score(z.beam[i][1], z.beam[i][2], z.E) for i in live])
                else:
                    score.append([total_score(tf[i], z.E) for i in live])
            else:
                live = [0]
                score.append([F(-np.inf)])
            hyp.append([z.prefix(z.beam[i][0]) for i in live])
            count.append(len(live))
            alive = [z.prefix(nd) for i, (nd, _, _) in enumerate(z.beam) if tot[i] > 0]
            stable.append(common_prefix_len(alive) if alive else len(z.prefix(z.beam[0][0])))
        return dict(hyp=hyp, score=score, nbest_count=count, frames=frames, stable_len=stable)
