"""The numpy twin of klstm_ctc_align (include/klstm.h; tests/test_ctc_align.py, tests/test_ctc_align_gpu.py), host only.  The twin IS the
definition of the call.
  emissions()         log(max(float32(y * w), FLT_MIN)) of the lattice states of one utterance, a NaN counts as FLT_MIN
  align_twin()        Viterbi over the CTC lattice (states 0 .. 2L, even = blank, odd i = label i >> 1; start in 0 or 1, end in 2L or
                      2L - 1; stay / advance / skip onto a label that differs from the one before).  Ties: stay, then advance, then
                      skip; at the end 2L over 2L - 1.  dtype=np.float64 is the definition; dtype=np.float32 is the STOCK fp32 chain
                      (numpy float32 log, unnormalised float32 running sums): the yardstick of the optimality bar
  best_brute_force()  the best score over ALL K^T paths that collapse to the labels, float64, for tiny cases: pins the twin
                      independently of its own recurrence
  validate()          the structural checks of an alignment: collapses to the labels, positions monotone, token bounds a partition
                      consistent with frame_pos
  path_score64()      the float64 sum of the unweighted emissions along a frame_class path"""
import itertools

import numpy as np

from tests.ctc_decode_ref import collapse

FLT_MIN = np.float32(np.finfo(np.float32).tiny)
IDLE, ALIGNED, REJECTED = 0, 1, 2


def status(n, T, lab, K, blank, max_labels=1023):
    """what klstm_ctc_eval and klstm_ctc_align decide on the device"""
    if n == 0:
        return IDLE
    lab = list(lab)
    rep = sum(1 for a, b in zip(lab[:-1], lab[1:]) if a == b)
    if n < 0 or n > T or len(lab) > max_labels or any(c < 0 or c >= K or c == blank for c in lab) or n < len(lab) + rep:
        return REJECTED
    return ALIGNED


def emissions(y, ext, w=None, dtype=np.float64):
    """y [n, K] float32 (valid frames) -> [n, len(ext)] of `dtype`"""
    y = np.asarray(y, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        v = y[:, ext] if w is None else (y[:, ext] * np.asarray(w, np.float32)[ext][None, :]).astype(np.float32)
    v = np.where(np.isnan(v), FLT_MIN, np.maximum(v, FLT_MIN)).astype(np.float32)
    with np.errstate(divide="ignore"):
        return np.log(v.astype(dtype))                      # float32 in, float32 log: the stock chain


def viterbi(em, skip):
    """em [n, N] log emissions (float64 or float32: the sums run in em.dtype), skip [N] bool -> (states [n], best)"""
    n, N = em.shape
    dt = em.dtype.type
    ninf = dt(-np.inf)
    v = np.full(N, ninf, em.dtype)
    v[:2] = em[0, :2]
    bp = np.zeros((n, N), np.int8)
    for t in range(1, n):
        pad = np.concatenate([[ninf, ninf], v])
        x1, x2 = pad[1:N + 1], np.where(skip, pad[:N], ninf)
        m, mv = v, np.zeros(N, np.int8)
        c = x1 > m
        m, mv = np.where(c, x1, m), np.where(c, 1, mv)
        c = x2 > m
        m, mv = np.where(c, x2, m), np.where(c, 2, mv)
        bp[t] = mv
        with np.errstate(invalid="ignore"):
            v = (m + em[t]).astype(em.dtype)
    st = N - 1
    if N > 1 and v[N - 2] > v[N - 1]:
        st = N - 2
    best = v[st]
    states = np.empty(n, np.int64)
    for t in range(n - 1, -1, -1):
        states[t] = st
        st -= int(bp[t, st])
    return states, best


def align_twin(y, lens, labels, blank, w=None, dtype=np.float64, max_labels=1023):
    """y [T, S, K] float32.  Returns a list of S dicts: status, state [n], frame_class [T], frame_pos [T] (-1 beyond n and for streams
    not aligned), token_begin [L], token_end [L] (-1 for streams not aligned), best (the chain's own score of its path, in `dtype`;
    None for streams not aligned)."""
    y = np.asarray(y, dtype=np.float32)
    T, S, K = y.shape
    out = []
    for s in range(S):
        n, lab = int(lens[s]), [int(c) for c in labels[s]]
        L = len(lab)
        r = dict(status=status(n, T, lab, K, blank, max_labels), state=np.zeros(0, np.int64), frame_class=np.full(T, -1, np.int32),
                 frame_pos=np.full(T, -1, np.int32), token_begin=np.full(L, -1, np.int32), token_end=np.full(L, -1, np.int32), best=None)
        out.append(r)
        if r["status"] != ALIGNED:
            continue
        N = 2 * L + 1
        ext = np.full(N, blank, np.int64)
        ext[1::2] = lab
        skip = np.zeros(N, bool)
        if L > 1:
            skip[3::2] = np.asarray(lab[1:]) != np.asarray(lab[:-1])
        states, best = viterbi(emissions(y[:n, s], ext, w, dtype), skip)
        r["state"], r["best"] = states, float(best)
        r["frame_class"][:n] = ext[states]
        pos = np.where(states & 1, states >> 1, -1)
        r["frame_pos"][:n] = pos
        for t in range(n):
            j = pos[t]
            if j >= 0:
                if t == 0 or pos[t - 1] != j:
                    r["token_begin"][j] = t
                if t == n - 1 or pos[t + 1] != j:
                    r["token_end"][j] = t + 1
    return out


def best_brute_force(y, labels, blank):
    """max over all T-frame paths that collapse to `labels` of sum_t log(max(y[t, path[t]], FLT_MIN)), float64; None if there is none.
    y [T, K]."""
    T, K = y.shape
    em = emissions(y, np.arange(K))
    best = None
    for path in itertools.product(range(K), repeat=T):
        if collapse(path, blank) == list(labels):
            sc = float(sum(em[t, path[t]] for t in range(T)))
            best = sc if best is None or sc > best else best
    return best


def path_score64(y_s, frame_class):
    """y_s [n, K] float32, frame_class [n] -> the float64 sum of the unweighted emissions along the path"""
    n = len(frame_class)
    return float(emissions(y_s[:n], np.arange(y_s.shape[1]))[np.arange(n), np.asarray(frame_class, np.int64)].sum())


def validate(frame_class, frame_pos, token_begin, token_end, labels, blank):
    """frame_class, frame_pos over the n valid frames of one aligned utterance; token_begin, token_end over its labels.  Raises
    AssertionError with the reason."""
    fc, fp = [int(c) for c in frame_class], [int(p) for p in frame_pos]
    lab, L, n = [int(c) for c in labels], len(labels), len(fc)
    assert collapse(fc, blank) == lab, "the path does not collapse to the labels"
    for t in range(n):
        assert (fp[t] == -1) == (fc[t] == blank), f"frame {t}: position {fp[t]} with class {fc[t]}"
        assert fp[t] == -1 or (0 <= fp[t] < L and lab[fp[t]] == fc[t]), f"frame {t}: class {fc[t]} at position {fp[t]}"
    seen = [p for p in fp if p >= 0]
    assert all(b - a in (0, 1) for a, b in zip(seen[:-1], seen[1:])), "positions are not monotone"
    assert sorted(set(seen)) == list(range(L)), "a label position has no frame"
    tb, te = [int(v) for v in token_begin], [int(v) for v in token_end]
    prev_end = 0
    for j in range(L):
        assert prev_end <= tb[j] < te[j] <= n, f"token {j}: [{tb[j]}, {te[j]}) after {prev_end}"
        assert all(fp[t] == j for t in range(tb[j], te[j])), f"token {j}: a frame inside its bounds belongs elsewhere"
        assert all(fp[t] == -1 for t in range(prev_end, tb[j])), f"token {j}: a label frame before its begin"
        prev_end = te[j]
    assert all(p == -1 for p in fp[prev_end:]), "a label frame after the last token's end"


# ---------------------------------------------------------------------------------------------------------------------------------
# the inputs of the EXACT comparisons of tests/test_ctc_align_gpu.py: posteriors peaked on an alignment (any deviation from the best
# path costs of the order of log K nats, orders of magnitude above float32 rounding) and uniform ones (exact ties).  tests/
# test_ctc_align.py checks on the CPU that the stock float32 chain and the float64 chain agree on every one of them.
# ---------------------------------------------------------------------------------------------------------------------------------
def random_labels(rng, K, blank, n, repeat=True):
    """n labels other than the blank; with `repeat`, one adjacent pair of equal labels in the middle"""
    lab = rng.randint(0, K - 1, n)
    lab = (lab + (lab >= blank)).tolist()
    if repeat and n >= 2:
        lab[n // 2] = lab[n // 2 - 1]
    return lab


def peaked(seed, T, K, blank, lens, lab_lens, corrupt=(0, 0, 0, 0)):
    """-> (y [T, S, K], labels): tests/ctc_decode_ref.peaked_case on seeded labels, every stream corrupted by `corrupt`"""
    from tests.ctc_decode_ref import peaked_case
    rng = np.random.RandomState(seed)
    labels = [random_labels(rng, K, blank, n) for n in lab_lens]
    return peaked_case(seed, T, K, blank, labels, lens, [tuple(corrupt)] * len(lens)), labels


def mild_weights(seed, K):
    return (2.0 ** np.random.RandomState(seed).uniform(-2, 2, K)).astype(np.float32)


def _case(y, lens, labels, blank=0, w=None):
    return dict(y=y, lens=list(lens), labels=labels, blank=blank, w=w)


def _pk(seed, T, K, blank, lens, lab_lens, corrupt=(0, 0, 0, 0), w=None):
    y, labels = peaked(seed, T, K, blank, lens, lab_lens, corrupt)
    return _case(y, lens, labels, blank, w)


EXACT_CASES = {}


def _register():
    E = EXACT_CASES
    lens_a, labs_a = [300, 250, 120, 30], [60, 50, 40, 10]
    for seed in (11, 12):
        E[f"peaked{seed}"] = lambda seed=seed: _pk(seed, 300, 48, 0, lens_a, labs_a)
        E[f"peaked{seed}_corrupted"] = lambda seed=seed: _pk(seed, 300, 48, 0, lens_a, labs_a, (3, 2, 2, 1))
    E["peaked11_weighted"] = lambda: _pk(11, 300, 48, 0, lens_a, labs_a, w=mild_weights(11, 48))

    def uniform():
        y = np.full((20, 4, 64), 1.0 / 64, np.float32)
        return _case(y, [20, 20, 7, 20], [[5, 5, 9], [], [1, 1, 1, 1], [3]], 0)       # stream 2: len == L + repeats exactly
    E["uniform"] = uniform
    for K in (2, 29, 64, 65, 4097, 16624, 32768):
        T = 40 if K <= 4097 else 12
        lens, lab_lens = [T, T - 3, 0, T // 2, 1], ([7, 0, 3, 5, 1] if K <= 4097 else [3, 0, 2, 2, 1])
        for blank in sorted({0, K // 2, K - 1}):
            E[f"K{K}_blank{blank}"] = lambda K=K, T=T, lens=lens, lab_lens=lab_lens, blank=blank: \
                _pk(K + blank, T, K, blank, lens, lab_lens)
        E[f"K{K}_weighted"] = lambda K=K, T=T, lens=lens, lab_lens=lab_lens: \
            _pk(K, T, K, K // 2, lens, lab_lens, w=mild_weights(K, K))
    for S in (1, 4, 15, 32):
        lens = [120 - (37 * s) % 60 for s in range(S)]
        E[f"S{S}"] = lambda S=S, lens=lens: _pk(S, 120, 29, 0, lens, [10 + (7 * s) % 16 for s in range(S)])
    for L in (31, 32, 127, 128, 255, 256, 511, 512, 1023):           # either side of 64 / 256 / 512 / 1024 states, and 2047
        T = 3 * L // 2 + 300
        E[f"L{L}"] = lambda L=L, T=T: _pk(L, T, 48, 0, [T, T - 37], [L, L - 1])
    # utterance lengths either side of the trace's blocks of 256 frames
    E["trace_blocks"] = lambda: _pk(5, 513, 29, 0, [255, 256, 257, 512, 513], [40] * 5)
    E["row_limit"] = lambda: _pk(6, 65535, 4, 0, [65535], [200])

    def nan_on_valid_frames():
        c = _pk(11, 300, 48, 0, lens_a, labs_a)
        c["y"][50, 0, :] = np.nan                                     # a whole valid row: every emission FLT_MIN
        c["y"][10, 1, c["labels"][1][0]] = np.nan
        return c
    E["nan_on_valid_frames"] = nan_on_valid_frames

    def statuses(short):
        """idle, every reason to reject, L = 0, len == L + repeats exactly (streams 8, 10) and one frame short of it"""
        from tests.ctc_decode_ref import peaked_case
        K, T, blank = 32, 200, 3
        rng = np.random.RandomState(9)
        lens = [200, 0, 201, -1, 200, 200, 200, 150, 39, 40, 41]
        labs = [random_labels(rng, K, blank, 20) for _ in lens]
        labs[4][4] = K                                                  # outside [0, K)
        labs[5][0] = blank                                              # the blank itself
        labs[6] = []                                                    # all blank
        labs[8], labs[9], labs[10] = [7] * 20, [7] * 20, [7] * 21        # 39, 39 and 41 frames needed
        fine = [lab if all(0 <= c < K and c != blank for c in lab) else [5] for lab in labs]
        y = peaked_case(9, T, K, blank, fine, [n if 0 < n <= T else 0 for n in lens], [(0, 0, 0, 0)] * len(lens))
        y[:, 2] = y[:, 0]
        y[:, 3] = y[:, 0]
        if short:
            lens[8] = 38
        return _case(y, lens, labs, blank)
    E["statuses"] = lambda: statuses(False)
    E["statuses_one_frame_short"] = lambda: statuses(True)

    def padding(fill):
        """what padding rows, idle and rejected streams hold does not matter: they are not read"""
        lens = [60, 0, 41, 7, 60, 61]                                   # stream 5: longer than T, rejected
        c = _pk(3, 60, 300, 0, [60, 60, 41, 7, 60, 60], [10, 4, 9, 2, 0, 5], w=mild_weights(3, 300))
        for s, n in enumerate(lens):
            c["y"][(n if n <= 60 else 0):, s] = fill
        c["lens"] = lens
        return c
    for name, fill in (("zero", 0.0), ("nan", np.nan), ("inf", np.inf), ("huge", 1e38)):
        E[f"padding_{name}"] = lambda fill=fill: padding(fill)
    E["capacity_9_labels"] = lambda: _pk(3, 60, 29, 0, [60, 60, 50], [5, 9, 4])
    E["capacity_17_labels"] = lambda: _pk(4, 60, 29, 0, [60, 60, 50], [5, 17, 4])


_register()
