"""The numpy twin of klstm_ctc_beam_stream_step / klstm_ctc_beam_stream_emit (include/klstm.h; tests/test_ctc_beam_stream.py,
tests/test_ctc_beam_stream_gpu.py), host only: the search of tests/ctc_beam_ref.py / tests/ctc_beam_lm_ref.py fed chunk by chunk.  The
twin IS the definition.  Per stream it holds what the device holds, a Stream of tests/ctc_beam_ref.py: the prefix tree (parent, token,
length, hash, LM state per node), the beam (node, pb, pnb), the exponent E and the frames consumed.  The frames are run by frame()
of that file, the one the whole-utterance twins run, and the lists are made by its nbest_list(); what is defined here:
  step()           lens[s] frames of a chunk [T, S, K] per stream; 0 is idle (the state is not touched, even with start set); start[s]
                   begins a new utterance; state that was never started starts at its first non-idle step; a stream whose frames
                   would exceed max_frames is rejected for the call, its state unchanged but for the sticky overflow flag
  emit()           per stream and mode (0 skip, 1 without the final weights, 2 with them) the list beam_twin / beam_twin_lm make of
                   the beam, frames (-1 - frames after an overflow) and stable_len
  stable_len       computed the obvious way: the longest common prefix of the token lists of all beam entries with a total > 0; a
                   DEAD beam: the length of its first entry"""
import numpy as np

from tests.ctc_beam_lm_ref import lm_tables
from tests.ctc_beam_ref import Stream, beam_totals, emissions, frame, nbest_list


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
                self.z[s] = Stream()
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
            tot = beam_totals(z.beam)
            fin = self.fin if mode[s] == 2 else None
            live, sc = nbest_list(tot, z.E, nbest, None if fin is None else [fin[z.st[nd]] for nd, _, _ in z.beam])
            hyp.append([z.prefix(z.beam[i][0]) for i in live]); score.append(sc); count.append(len(live))
            alive = [z.prefix(nd) for i, (nd, _, _) in enumerate(z.beam) if tot[i] > 0]
            stable.append(common_prefix_len(alive) if alive else len(z.prefix(z.beam[0][0])))
        return dict(hyp=hyp, score=score, nbest_count=count, frames=frames, stable_len=stable)
