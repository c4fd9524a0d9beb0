"""The numpy twin of klstm_ctc_nbest_rescore (include/klstm.h; kaldi-lstm_amd/csrc/klstm_ctc_rescore.hip), host only:
second-pass rescoring of n-best lists with sparse back-off models over tokens and words.  rescore() is the twin: every product, frexp
and sum in the order the device takes it, so that the mantissa and the exponent of a walk carry the device's bits and only the one log
may differ.  brute() is an independent brute force (weights from the dense expansion of the model, math.fsum of math.log, Python
sorted) that tests/test_ctc_rescore.py holds the twin against.  The units and their keys are those of tests/ctc_consensus_ref.py."""
import math

import numpy as np

import kaldi_lstm_amd.lm as LM
from kaldi_lstm_amd.lm import word_sequences, word_table
from tests.ctc_consensus_ref import units_of, word_key  # noqa: F401  (word_key: for the tests)
from tests.nbest_ref import pack

TOTALS = 8
LN2 = 0.6931471805599453
F32 = np.float32


def flush(v):
    """the emission rule: NaN or below 2^-60 is exactly 0, above 2^60 is 2^60"""
    return LM._flush(v, F32)


class Words:
    """a word table as the device sees it: keys uint64 [W], ids int32 [W] (sorted or not), unk_id, separator"""

    def __init__(self, keys, ids, unk_id, separator):
        self.keys, self.ids = [int(k) for k in keys], [int(i) for i in ids]
        self.unk_id, self.separator = int(unk_id), int(separator)

    def lookup(self, k, V, reserved):
        """-> (class or -1: forbids, out of vocabulary?) by THE bisection, whatever order the keys are in"""
        W = len(self.keys)
        lo, hi = 0, W
        while lo < hi:
            mid = (lo + hi) >> 1
            if self.keys[mid] < k:
                lo = mid + 1
            else:
                hi = mid
        i = self.ids[lo] if lo < W and self.keys[lo] == k else -1
        if i < 0 or i >= V or i == reserved:
            return (self.unk_id if self.unk_id >= 0 else -1), True
        return i, False


def walk(lm, units, depths=None):
    """the walk of a sparse model over units from state 0 -> (forbidden, m, e, logw); logw = -inf when forbidden.  depths: a list the
    back-off depth of every lookup is appended to"""
    Q = len(lm.backoff)
    m, e, q = np.float64(1.0), 0, 0
    for u in units:
        if u < 0:
            return True, m, e, -np.inf
        g, nx, d = LM.sparse_lm_lookup(lm, q, int(u), with_depth=True)
        if depths is not None:
            depths.append(d)
        gf = flush(g)
        if gf == 0 or nx < 0 or nx >= Q:
            return True, m, e, -np.inf
        m, de = np.frexp(m * np.float64(gf))
        e, q = e + int(de), nx
    if lm.final is not None:
        gf = flush(lm.final[q])
        if gf == 0:
            return True, m, e, -np.inf
        m, de = np.frexp(m * np.float64(gf))
        e += int(de)
    return False, m, e, np.log(m) + np.float64(e) * np.float64(LN2)


def rescore(hyp, hyp_len, count, logp, K, sub=None, add=None, words=None, add_reserved=-1, am_scale=1.0, add_scale=1.0, unit_bonus=0.0,
            errors=None, max_len=None, out_n=None, out_stride=None, depths=None):
    """-> dict of numpy arrays named as the C entry names them (order, live_count, score, add_logp, sub_logp, units, oov, out_hyp,
    out_len, out_count, out_score, out_errors), plus totals [8] (what ONE call adds), z64 [S, N] (nan: not ranked), status [S]"""
    hyp, hyp_len, count = np.asarray(hyp), np.asarray(hyp_len), np.asarray(count)
    logp = np.asarray(logp, dtype=F32)
    S, N, stride = hyp.shape
    max_len = min(1023, stride) if max_len is None else max_len
    out_n = N if out_n is None else out_n
    out_stride = max(min(stride, max_len), 1) if out_stride is None else out_stride
    am, asc, ub = (np.float64(F32(v)) for v in (am_scale, add_scale, unit_bonus))
    V = add.classes if add is not None else 0
    o = dict(order=np.full((S, N), -1, np.int32), live_count=np.zeros(S, np.int32), score=np.full((S, N), -np.inf, F32),
             add_logp=np.full((S, N), -np.inf, F32), sub_logp=np.full((S, N), -np.inf, F32), units=np.zeros((S, N), np.int32),
             oov=np.zeros((S, N), np.int32), z64=np.full((S, N), np.nan), status=[],
             out_hyp=np.zeros((S, max(out_n, 1), out_stride), np.int32), out_len=np.zeros((S, max(out_n, 1)), np.int32),
             out_count=np.zeros(S, np.int32), out_score=np.full((S, max(out_n, 1)), -np.inf, F32),
             out_errors=np.full((S, max(out_n, 1)), -1, np.int32))
    tot = np.zeros(TOTALS)
    for s in range(S):
        c = int(count[s])
        if c < 0 or c > N:
            o["status"].append("rejected")
            tot[1] += 1
            continue
        z = {}
        for q in range(c):
            n = int(hyp_len[s, q])
            ok = bool(np.isfinite(logp[s, q])) and 0 <= n <= min(stride, max_len)
            toks = hyp[s, q, :n].tolist() if ok else []
            if not ok or any(t < 0 or t >= K for t in toks):
                tot[2] += 1
                continue
            if words is None:
                units = toks
            else:
                units = []
                for k in units_of(toks, words.separator):
                    i, is_oov = words.lookup(k, V, add_reserved)
                    units.append(i)
                    o["oov"][s, q] += is_oov
            o["units"][s, q] = len(units)
            tot[7] += o["oov"][s, q]
            f_sub, _, _, lw_sub = walk(sub, toks) if sub is not None else (False, 1.0, 0, np.float64(0.0))
            f_add, _, _, lw_add = walk(add, units, depths) if add is not None else (False, 1.0, 0, np.float64(0.0))
            o["sub_logp"][s, q], o["add_logp"][s, q] = lw_sub, lw_add
            if f_sub or f_add:
                tot[3] += 1
                continue
            v = am * np.float64(logp[s, q])
            if sub is not None:
                v = v - lw_sub
            if add is not None:
                v = v + asc * lw_add
            v = v + ub * np.float64(len(units))
            z[q] = v + np.float64(0.0)
            o["z64"][s, q], o["score"][s, q] = z[q], z[q]
        ranked = sorted(z, key=lambda q: (-z[q], q))
        o["live_count"][s] = len(ranked)
        o["order"][s, :len(ranked)] = ranked
        if out_n >= 1:
            o["out_count"][s] = min(len(ranked), out_n)
            for r, q in enumerate(ranked[:out_n]):
                n = int(hyp_len[s, q])
                o["out_hyp"][s, r, :n], o["out_len"][s, r], o["out_score"][s, r] = hyp[s, q, :n], n, z[q]
                if errors is not None:
                    o["out_errors"][s, r] = errors[s, q]
        if not ranked:
            o["status"].append("idle")
            tot[1] += 1
            continue
        o["status"].append("done")
        tot[0] += 1
        tot[4] += ranked[0] != 0
        if errors is not None:
            tot[5] += int(errors[s, 0])
            tot[6] += int(errors[s, ranked[0]])
    o["totals"] = tot
    return o


def brute(lists, logps, sub=None, add=None, words=None, vocab=None, unk_id=-1, separator=-1, am_scale=1.0, add_scale=1.0, unit_bonus=0.0):
    """ONE stream of well-formed entries, independently: the weights of a model from its dense expansion (sparse_lm_to_dense), the log
    weight as math.fsum of math.log, words as tuples of tokens looked up in the dict `vocab` (no hash, no bisection), Python sorted.
    -> dict(z: per entry a float or None where forbidden, sub_logw, add_logw, order)"""
    def logw(dense, units):
        nxt, wt, fin = dense
        q, terms = 0, []
        for u in units:
            if u < 0:
                return None
            g = float(wt[q, u])
            if not (g >= 2.0 ** -60) or nxt[q, u] < 0:
                return None
            terms.append(math.log(min(g, 2.0 ** 60)))
            q = int(nxt[q, u])
        if fin is not None:
            g = float(fin[q])
            if not (g >= 2.0 ** -60):
                return None
            terms.append(math.log(min(g, 2.0 ** 60)))
        return math.fsum(terms)
    d_sub = LM.sparse_lm_to_dense(sub) if sub is not None else None
    d_add = LM.sparse_lm_to_dense(add) if add is not None else None
    zs, subs, adds = [], [], []
    for toks, lp in zip(lists, logps):
        if separator < 0:
            units = list(toks)
        else:
            units, cur = [], []
            for t in list(toks) + [separator]:
                if t == separator:
                    if cur:
                        units.append(vocab.get(tuple(cur), unk_id))
                    cur = []
                else:
                    cur.append(t)
        ls = logw(d_sub, toks) if sub is not None else 0.0
        la = logw(d_add, units) if add is not None else 0.0
        subs.append(ls)
        adds.append(la)
        if ls is None or la is None:
            zs.append(None)
            continue
        zs.append(float(F32(am_scale)) * float(F32(lp)) - ls + float(F32(add_scale)) * la + float(F32(unit_bonus)) * len(units))
    order = sorted((q for q in range(len(zs)) if zs[q] is not None), key=lambda q: (-zs[q], q))
    return dict(z=zs, sub_logw=subs, add_logw=adds, order=order)


def min_gap(o, skip=()):
    """the smallest relative gap between adjacent ranked z over the streams not in `skip`"""
    g = np.inf
    for s in range(len(o["live_count"])):
        if s in skip:
            continue
        z = o["z64"][s, o["order"][s, :o["live_count"][s]]]
        for a, b in zip(z[:-1], z[1:]):
            g = min(g, (a - b) / max(abs(a), abs(b), 1e-300))
    return g


# ------------------------------------------------------------------------------------------------------------------------------------
# the inputs of the tests (host and GPU): models and lists
# ------------------------------------------------------------------------------------------------------------------------------------
def token_corpus(seed, K, n=60, L=14, blank=0):
    """label sequences with structure: a first-order chain with a few favoured successors per class, so that high orders are seen"""
    rng = np.random.default_rng(seed)
    fav = {c: rng.choice([k for k in range(K) if k != blank], size=3, replace=False) for c in range(K)}
    out = []
    for _ in range(n):
        c = int(rng.integers(1, K))
        seq = [c]
        for _ in range(int(rng.integers(L // 2, L + 1)) - 1):
            c = int(rng.choice(fav[c])) if rng.random() < 0.8 else int(rng.choice([k for k in range(K) if k != blank]))
            seq.append(c)
        out.append(seq)
    return out


def token_models(K=12, blank=0, seed=7):
    """(corpus, bigram, order-4 model): absolute-discounting back-off models over the corpus.  At K = 12 every state of the bigram has at
    least K / 4 arcs (a direct row on the device); the order-4 model's deep states have fewer (bisected)"""
    corpus = token_corpus(seed, K, blank=blank)
    return corpus, LM.backoff_ngram_label_lm(corpus, K, blank, order=2), LM.backoff_ngram_label_lm(corpus, K, blank, order=4)


def lists_from_corpus(seed, corpus, S, N, K, blank=0, stride=None, spread=6.0):
    """per stream a corpus sentence, every entry 0-3 edits of it (distinct); logp sorted draws, best first"""
    rng = np.random.default_rng(seed)
    rows = []
    for s in range(S):
        base = list(corpus[int(rng.integers(0, len(corpus)))])
        ent = []
        for q in range(N):
            for _ in range(1000):
                h = list(base)
                for _ in range(int(rng.integers(0, 4)) if q else 0):
                    kind, pos = int(rng.integers(0, 3)), int(rng.integers(0, len(h) + 1))
                    tok = int(rng.choice([k for k in range(K) if k != blank]))
                    if kind == 0 and h:
                        h[min(pos, len(h) - 1)] = tok
                    elif kind == 1 and len(h) > 1:
                        del h[min(pos, len(h) - 1)]
                    elif kind == 2:
                        h.insert(pos, tok)
                if h not in ent:
                    break
            assert h not in ent
            ent.append(h)
        rng.shuffle(ent)
        rows.append(ent)
    return pack(rows, stride) + (-np.sort(spread * rng.random((S, N)), axis=1).astype(F32),)


def word_setup(seed=3, K=8, nwords=30, sep=0):
    """a vocabulary of `nwords` words of 1-4 tokens over the classes 1 .. K - 1 (0 the separator), sentences over it, and a word trigram:
    V = nwords + 2 classes, nwords the class of unknown words, nwords + 1 reserved.  -> dict(vocab, table, sents, model, V, unk, reserved,
    sep, K)"""
    rng = np.random.default_rng(seed)
    vocab = []
    while len(vocab) < nwords:
        w = rng.integers(1, K, size=int(rng.integers(1, 5))).tolist()
        if w not in vocab:
            vocab.append(w)
    unk, reserved, V = nwords, nwords + 1, nwords + 2
    table = word_table(vocab, sep)
    fav = {i: rng.choice(nwords, size=3, replace=False) for i in range(nwords)}
    sents = []
    for _ in range(80):
        i = int(rng.integers(0, nwords))
        snt = [i]
        for _ in range(int(rng.integers(2, 7))):
            i = int(rng.choice(fav[i])) if rng.random() < 0.8 else int(rng.integers(0, nwords))
            snt.append(i)
        sents.append(snt)
    label_seqs = [sum((vocab[i] + [sep] for i in snt), [])[:-1] for snt in sents]
    label_seqs.append([7, 7, 7, 7, 7, sep] + vocab[0])                   # an unknown word in the training data: the class unk is seen
    seqs = word_sequences(label_seqs, table, sep, unk)
    model = LM.backoff_ngram_label_lm(seqs, V, reserved, order=3)
    return dict(vocab=vocab, table=table, sents=sents, model=model, V=V, unk=unk, reserved=reserved, sep=sep, K=K)


def word_lists(ws, seed=0, S=3, N=8):
    """word-level edits of one sentence per stream, with leading, trailing and doubled separators, unknown words, and one entry of
    separators alone"""
    rng = np.random.default_rng(seed)
    sep, vocab = ws["sep"], ws["vocab"]
    rows = []
    for s in range(S):
        base = [vocab[i] for i in ws["sents"][s]]
        ent = []
        for q in range(N):
            words = [list(w) for w in base]
            for _ in range(int(rng.integers(0, 3)) if q else 0):
                kind, pos = int(rng.integers(0, 3)), int(rng.integers(0, len(words)))
                if kind == 0:
                    words[pos] = vocab[int(rng.integers(0, len(vocab)))]
                elif kind == 1 and len(words) > 1:
                    del words[pos]
                else:
                    words.insert(pos, rng.integers(1, ws["K"], size=5).tolist())        # five tokens: no word of the vocabulary
            toks = [sep] * int(rng.integers(0, 3))
            for w in words:
                toks += list(w) + [sep] * (2 if rng.random() < 0.25 else 1)
            if rng.random() < 0.5:
                toks = toks[:-1]
            ent.append(toks)
        rows.append(ent)
    rows[1][5] = [sep] * 4
    hyp, hyp_len, count = pack(rows, stride=max(len(t) for e in rows for t in e) + 3)
    logp = -np.sort(6.0 * rng.random((S, N)), axis=1).astype(F32)
    return hyp, hyp_len, count, logp


def forbidding_model():
    """K = 4, two states.  State 0: 1 -> state 1 (0.5), 2 -> state 0 with weight 0, 3 -> a next outside [0, Q); state 1: 1 -> state 0
    and nothing else, no back-off; final (0.5, 0)"""
    return LM.SparseLm(4, np.array([0, 3, 4], np.int32), np.array([1, 2, 3, 1], np.int32), np.array([1, 0, 5, 0], np.int32),
                      np.array([0.5, 0.0, 0.25, 0.5], np.float32), np.array([-1, -1], np.int32), np.ones(2, np.float32),
                      np.array([0.5, 0.0], np.float32))
