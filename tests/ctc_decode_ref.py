"""The numpy twin of klstm_ctc_decode (include/klstm.h; tests/test_ctc_decode.py, tests/test_ctc_decode_gpu.py), host only.  The twin IS
the definition; every integer the kernel produces must equal it exactly.
  frame_classes()  per valid row: argmax over k of key(float32(y[k] * w[k])), key(NaN) = -inf, ties to the lowest column; -1 elsewhere
  collapse()       drop repeats, then blanks
  levenshtein()    the plain two-row recurrence (substitution, insertion, deletion cost 1)
  decode_twin()    everything klstm_ctc_decode returns except the score, with the stream statuses of the header
  path_logp64()    the float64 sum of log(max(y_best, FLT_MIN)) over the twin's path: what `score` is measured against
  peaked_case()    posteriors peaked on a known alignment of a reference, corrupted by a seeded number of substitutions, deletions,
                   insertions and repeats-without-blank: hypotheses CLOSE to their references"""
import numpy as np

from tests.nbest_ref import levenshtein  # noqa: F401  (the tests take it from here)

FLT_MIN = np.float32(np.finfo(np.float32).tiny)


def frame_classes(y, lens, w=None):
    """y [T, S, K] float32 -> int32 [T, S]"""
    y = np.asarray(y, dtype=np.float32)
    T, S, K = y.shape
    out = np.full((T, S), -1, np.int32)
    for s in range(S):
        n = lens[s]
        if n <= 0 or n > T:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            v = y[:n, s] if w is None else (y[:n, s] * np.asarray(w, np.float32)[None, :]).astype(np.float32)
        key = np.where(np.isnan(v), -np.inf, v)
        out[:n, s] = np.argmax(key, axis=1)                 # numpy: the first of equal maxima
    return out


def collapse(path, blank):
    out, prev = [], None
    for t, c in enumerate(path):
        c = int(c)
        if c != blank and (t == 0 or c != prev):
            out.append(c)
        prev = c
    return out


def decode_twin(y, lens, blank, w=None, refs=None):
    """-> dict(frame_class [T, S], hyp [S lists], errors [S] or None, totals [5] or None)"""
    y = np.asarray(y, dtype=np.float32)
    T, S, K = y.shape
    fc = frame_classes(y, lens, w)
    hyp = [collapse(fc[:lens[s], s], blank) if 0 < lens[s] <= T else [] for s in range(S)]
    errors = totals = None
    if refs is not None:
        errors, totals = [-1] * S, [0.0] * 5
        for s in range(S):
            r = list(refs[s])
            if not 0 < lens[s] <= T or len(r) > 1023 or any(c < 0 or c >= K or c == blank for c in r):
                continue
            e = errors[s] = levenshtein(hyp[s], r)
            totals = [totals[0] + e, totals[1] + len(r), totals[2] + len(hyp[s]), totals[3] + 1, totals[4] + (e > 0)]
    return dict(frame_class=fc, hyp=hyp, errors=errors, totals=totals)


def path_logp64(y, lens, fc):
    """float64 sums of log(max(y[t, s, fc[t, s]], FLT_MIN)) over the valid frames (0 for idle / rejected streams)"""
    y = np.asarray(y, dtype=np.float32)
    T, S, _ = y.shape
    out = np.zeros(S)
    for s in range(S):
        n = lens[s]
        if 0 < n <= T:
            yb = y[np.arange(n), s, fc[:n, s]]
            out[s] = np.log(np.fmax(yb, FLT_MIN).astype(np.float64)).sum()
    return out


def path_logp32_stock(y, lens, fc):
    """the yardstick of the score's bar: numpy log in float32, summed sequentially in float32"""
    y = np.asarray(y, dtype=np.float32)
    T, S, _ = y.shape
    out = np.zeros(S, np.float32)
    for s in range(S):
        n = lens[s]
        if 0 < n <= T:
            lg = np.log(np.fmax(y[np.arange(n), s, fc[:n, s]], FLT_MIN))
            acc = np.float32(0)
            for v in lg:
                acc = np.float32(acc + v)
            out[s] = acc
    return out


def peaked_case(seed, T, K, blank, refs, lens, corrupt):
    """y [T, S, K] float32 whose best path of stream s is an alignment of refs[s] (every label a run of frames, a blank between equal
    neighbours and wherever room is left), after corrupt[s] = (substitutions, deletions, insertions, merges) seeded edits of the
    ALIGNED label sequence: a merge gives a token the class of the frame before it, with no blank between (repeat without blank).
    Rows beyond lens[s] are NaN.  The caller computes the expected distance with the twin; this only shapes the input."""
    rng = np.random.RandomState(seed)
    S = len(refs)
    y = np.full((T, S, K), np.nan, np.float32)
    classes = [c for c in range(K) if c != blank]
    for s in range(S):
        n = lens[s]
        if n <= 0:
            continue
        toks = list(refs[s])
        sub, dele, ins, mer = corrupt[s]
        for _ in range(sub):
            if toks:
                toks[rng.randint(len(toks))] = classes[rng.randint(len(classes))]
        for _ in range(dele):
            if toks:
                del toks[rng.randint(len(toks))]
        for _ in range(ins):
            toks.insert(rng.randint(len(toks) + 1), classes[rng.randint(len(classes))])
        merged = set(rng.choice(np.arange(1, max(2, len(toks))), size=min(mer, max(0, len(toks) - 1)), replace=False).tolist()) if mer else set()
        path = []
        for j, c in enumerate(toks):
            if j in merged:
                path.append(path[-1] if path else c)         # the class of the frame before, no blank between: collapses away
            else:
                if j > 0 and (toks[j - 1] == c or rng.rand() < 0.3):
                    path.append(blank)
                path.append(c)
        path = path[:n]
        reps = np.ones(len(path), np.int64)
        for _ in range(n - len(path)):                       # stretch runs (and leading blanks) to fill the utterance
            if len(path):
                reps[rng.randint(len(path))] += 1
        frames = np.repeat(np.asarray(path, np.int64), reps) if len(path) else np.zeros(0, np.int64)
        frames = np.concatenate([frames, np.full(n - len(frames), blank, np.int64)])
        p = rng.rand(n, K).astype(np.float32) * np.float32(0.5 / K)
        p[np.arange(n), frames] = np.float32(0.5) + rng.rand(n).astype(np.float32) * np.float32(0.4)
        y[:n, s] = p
    return y
