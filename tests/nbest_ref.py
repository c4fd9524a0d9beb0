"""What the host-side twins and tests of the n-best second pass share (tests/ctc_consensus_ref.py, tests/ctc_rescore_ref.py, their
host and GPU tests, and the decoders' twins): the hash a prefix or a word is known by, the word rule, the Levenshtein distance, the
packing of token lists into the arrays the device reads, the garbage written where the device may not read, and the distance of two
float32 arrays in ulps.  Independent of the product: numpy only, nothing from kaldi_lstm_amd."""
import numpy as np

H0, HMUL = 0x243F6A8885A308D3, 0x9E3779B97F4A7C15      # KLSTM_CTC_HASH_START, KLSTM_CTC_HASH_MUL of include/klstm.h
M64 = (1 << 64) - 1


def beam_hash(h, c):
    """one step of the hash: the device takes (unsigned)(c + 1)"""
    x = ((h ^ ((c + 1) & 0xFFFFFFFF)) * HMUL) & M64
    return x ^ (x >> 29)


def word_key(tokens):
    h = H0
    for c in tokens:
        h = beam_hash(h, int(c))
    return h


def split_words(tokens, separator):
    """the words of a token list: the maximal runs of tokens other than the separator (no empty words)"""
    out, word = [], []
    for t in list(tokens) + [separator]:
        if t != separator:
            word.append(int(t))
        elif word:
            out.append(word)
            word = []
    return out


def levenshtein(a, b):
    """two rows in numpy: D[j] = j + the running minimum of (tmp[j] - j), the device's row formulation, over any hashable units"""
    a, b = (a, b) if len(a) >= len(b) else (b, a)
    ids = {}
    cols = np.asarray([ids.setdefault(u, len(ids)) for u in a], dtype=np.int64)
    j = np.arange(len(a) + 1)
    prev = j.copy()
    for i, tok in enumerate(b, 1):
        tmp = np.empty_like(prev)
        tmp[0] = i
        tmp[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (cols != ids.get(tok, -1)))
        prev = j + np.minimum.accumulate(tmp - j)
    return int(prev[-1])


def pack(rows, stride=None, fill=0, len_fill=0):
    """[stream][entry] token lists -> hyp [S, N, stride], hyp_len [S, N], count [S]; fill, len_fill: what the unused tokens and the
    unused slots' lengths hold"""
    S, N = len(rows), max(len(e) for e in rows)
    stride = stride or max([len(h) for e in rows for h in e] + [1])
    hyp, hyp_len = np.full((S, N, stride), fill, np.int32), np.full((S, N), len_fill, np.int32)
    for s, ent in enumerate(rows):
        for q, h in enumerate(ent):
            hyp[s, q, :len(h)], hyp_len[s, q] = h, len(h)
    return hyp, hyp_len, np.array([len(e) for e in rows], np.int32)


def garbage(case):
    """10^6 in every token that may not be read, -7 / NaN in every list slot beyond the count"""
    hyp, hyp_len, count, logp = (np.array(case[k]) for k in ("hyp", "hyp_len", "count", "logp"))
    S, N, stride = hyp.shape
    for s in range(S):
        for q in range(N):
            if 0 <= count[s] <= N and q >= count[s]:
                hyp[s, q], hyp_len[s, q], logp[s, q] = 10 ** 6, -7, np.nan
            elif 0 <= hyp_len[s, q] <= stride:
                hyp[s, q, hyp_len[s, q]:] = 10 ** 6
    return dict(case, hyp=hyp, hyp_len=hyp_len, count=count, logp=logp)


def ulps(a, b):
    """the largest distance of two float32 arrays (or scalars) in ulps.  Asserted first: no NaN, infinities in the same places, the same
    signs in the same places"""
    a, b = np.ascontiguousarray(a, np.float32).ravel(), np.ascontiguousarray(b, np.float32).ravel()
    assert not np.isnan(a).any() and not np.isnan(b).any(), (a, b)
    assert np.array_equal(np.isinf(a), np.isinf(b)) and np.array_equal(a < 0, b < 0), (a, b)
    fin = np.isfinite(a)

    def ordered(v):
        i = v[fin].view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int(np.abs(ordered(a) - ordered(b)).max()) if fin.any() else 0
