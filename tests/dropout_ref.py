"""The numpy twin of include/klstm_dropout.h: Philox4x32-10, the threshold rule, the mask and the operator, written from the
header's definition and the published algorithm (Salmon, Moraes, Dror, Shaw 2011) alone.  Test infrastructure: the executable form
of the contract that kdrop_apply, the C++ <Dropout> layer and kaldi_lstm_amd.Dropout are held to, bit for bit."""
import numpy as np

ELEMENT, SEQUENCE = 0, 1
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Four uint32 words per counter; every argument broadcasts (arrays or ints below 2^32)."""
    c = [np.asarray(v, dtype=np.uint64) for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0), int(k1)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                       # < 2^64: exact in uint64
        c = [(p1 >> _32) ^ c[1] ^ np.uint64(k0), p1 & _LO, (p0 >> _32) ^ c[3] ^ np.uint64(k1), p0 & _LO]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def threshold(p):
    """(thr, scale) of a retention p, a float32 in [2^-32, 1]; None outside (NaN included)."""
    p = np.float32(p)
    if not (p >= np.float32(2.0 ** -32) and p <= np.float32(1)):
        return None
    thr = min(int(np.floor(float(p) * 4294967296.0)), 2 ** 32 - 1)
    return thr, np.float32(1) / p


def mask(rows, cols, p, seed, step, salt, mode=ELEMENT, S=1, seq_ids=None):
    """bool [rows, cols]: the elements kept"""
    assert 0 <= salt < 2 ** 31
    thr, _ = threshold(p)
    nq = (cols + 3) // 4
    q = np.arange(nq, dtype=np.uint64)[None, :]
    r = np.arange(rows, dtype=np.uint64)[:, None]
    if mode == ELEMENT:
        u, tag, st = r, salt, step & 0xFFFFFFFF
    else:
        u = np.asarray(seq_ids, dtype=np.uint64)[np.arange(rows) % S][:, None]
        tag, st = salt | 0x80000000, 0
    w = philox4x32_10(q, u, st, tag, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    words = np.stack(w, axis=-1).reshape(rows, nq * 4)[:, :cols]
    return words.astype(np.uint64) < np.uint64(thr)


def apply(x, p, seed, step, salt, mode=ELEMENT, S=1, seq_ids=None):
    """out = keep ? x * scale : +0.0 as float32; p == 1: x itself, bit for bit"""
    x = np.asarray(x, dtype=np.float32)
    if np.float32(p) == np.float32(1):
        return x.copy()
    _, scale = threshold(p)
    keep = mask(x.shape[0], x.shape[1], p, seed, step, salt, mode, S, seq_ids)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(keep, x * scale, np.float32(0)).astype(np.float32)
