"""Host helpers that build the tables of a label language model for ctc_beam_decode(lm=CtcLabelLm(...)) (klstm_ctc_beam_decode_lm of
include/klstm.h): a dense deterministic weighted automaton over the K classes.  State 0 is the start; label c leads
from state q to next[q, c] and multiplies the prefix probability by weight[q, c]; final[q] multiplies a hypothesis that ends in q.
numpy only.  Both builders return (next int32 [Q, K], weight float32 [Q, K], final float32 [Q]); the blank's column is never read
(next 0, weight 0).  Composing an n-gram with a lexicon (the product automaton) is the caller's.  Below them the SPARSE form
for back-off n-grams of higher order: its definition (sparse_lm_lookup), an ARPA reader and a count-based builder; and at the
end the words of the second pass (ctc_nbest_rescore): word_key, word_table, word_sequences, dense_lm_to_sparse."""
import collections
import math

import numpy as np


def ngram_states(K, order):
    """states of the n-gram automaton: 1 (order 1), 1 + K (order 2: 1 + c after label c), 1 + K + K^2 (order 3: 1 + K + a K + b after
    the labels a, b)"""
    assert order in (1, 2, 3), "order 1 to 3"
    return (1, 1 + K, 1 + K + K * K)[order - 1]


def ngram_next(K, order):
    """next [Q, K]: the history after one more label"""
    Q = ngram_states(K, order)
    nxt = np.zeros((Q, K), np.int32)
    c = np.arange(K)
    if order == 2:
        nxt[:] = 1 + c
    elif order == 3:
        nxt[0] = 1 + c
        for a in range(K):
            nxt[1 + a] = 1 + K + a * K + c
        last = np.arange(K * K) % K                          # state 1 + K + a K + b: the last label is b
        nxt[1 + K:] = 1 + K + last[:, None] * K + c[None, :]
    return nxt


def ngram_label_lm(sequences, K, blank, order=2, add_k=1.0, alpha=1.0, beta=0.0):
    """A dense add-k n-gram over label sequences (lists of classes other than the blank), order 1 to 3.  States are the histories
    (ngram_states); P(c | q) = (n(q, c) + add_k) / (n(q) + add_k * K) over the K - 1 labels and the end of the sequence, so a row and
    its end-of-sequence mass sum to 1.  weight = P(c | q)^alpha * e^beta: the LM weight alpha and the insertion bonus beta are folded
    in here; final = P(end | q)^alpha.  A history never seen with add_k = 0 forbids everything."""
    Q = ngram_states(K, order)
    nxt = ngram_next(K, order)
    cnt = np.zeros((Q, K), np.float64)
    end = np.zeros(Q, np.float64)
    for seq in sequences:
        q = 0
        for c in seq:
            c = int(c)
            assert 0 <= c < K and c != blank, "labels are classes other than the blank"
            cnt[q, c] += 1
            q = int(nxt[q, c])
        end[q] += 1
    den = cnt.sum(1) + end + add_k * K                       # K - 1 labels and the end of the sequence
    with np.errstate(all="ignore"):
        p = np.where(den[:, None] > 0, (cnt + add_k) / den[:, None], 0.0)
        pe = np.where(den > 0, (end + add_k) / den, 0.0)
    weight = np.where(p > 0, p ** alpha * math.exp(beta), 0.0)
    weight[:, blank] = 0.0
    nxt[:, blank] = 0
    return nxt, weight.astype(np.float32), np.where(pe > 0, pe ** alpha, 0.0).astype(np.float32)


def lexicon_label_lm(words, K, blank, separator):
    """The trie of `words` (each a non-empty list of classes other than the blank and the separator).  Inside a word only labels that
    continue some word are allowed (weight 1, everything else weight 0 and next -1); at the end of a word the separator returns to
    the root.  final is 1 at the end of a word and 0 elsewhere, so exactly the separator-joined sequences of one or more words are
    accepted."""
    assert 0 <= separator < K and separator != blank
    kids, is_end = [dict()], [False]
    for w in words:
        assert len(w) > 0, "no empty words"
        q = 0
        for c in w:
            c = int(c)
            assert 0 <= c < K and c != blank and c != separator, "word labels are classes other than the blank and the separator"
            if c not in kids[q]:
                kids[q][c] = len(kids)
                kids.append(dict()); is_end.append(False)
            q = kids[q][c]
        is_end[q] = True
    Q = len(kids)
    nxt = np.full((Q, K), -1, np.int32)
    weight = np.zeros((Q, K), np.float32)
    for q in range(Q):
        for c, q1 in kids[q].items():
            nxt[q, c] = q1
            weight[q, c] = 1.0
        if is_end[q]:
            nxt[q, separator] = 0
            weight[q, separator] = 1.0
    nxt[:, blank] = 0
    return nxt, weight, np.asarray(is_end, np.float32)


# ------------------------------------------------------------------------------------------------------------------------------------
# Sparse back-off models (klstm_ctc_slm_build / klstm_ctc_beam_decode_slm of include/klstm.h; ctc.CtcSparseLabelLm):
# a deterministic automaton with back-off arcs over the K classes, state 0 the start, the arcs of a state in CSR form with strictly
# ascending labels (never the blank), per state a back-off state (-1: none) and its weight, `final` dense as above.  Every back-off
# chain ends after at most SPARSE_MAX_BACKOFFS back-offs.
# ------------------------------------------------------------------------------------------------------------------------------------
SparseLm = collections.namedtuple("SparseLm", "classes arc_offsets arc_labels arc_next arc_weight backoff backoff_weight final")
SPARSE_MAX_BACKOFFS = 8


def _flush(v, dtype=np.float32):
    """the emission rule: NaN or below 2^-60 is exactly 0, above 2^60 is 2^60"""
    v = dtype(v)
    return min(v, dtype(2.0 ** 60)) if v >= dtype(2.0 ** -60) else dtype(0)


def sparse_lm_lookup(lm, q, c, with_depth=False, dtype=np.float32):
    """THE DEFINITION of a lookup (q, c) -> (g, n), which the device reproduces bit for bit: the arc of q for c gives its weight and
    its next; without one, and without a back-off, (0, -1): forbidden; else product = flush(product * flush(backoff_weight[q])), q =
    backoff[q], and again -- the product starts at 1 and multiplies the weight of the arc that is found after a back-off.  Every step
    is one multiplication in `dtype`.  with_depth: (g, n, back-offs taken)."""
    F = dtype
    prod = F(1)
    with np.errstate(all="ignore"):
        for depth in range(SPARSE_MAX_BACKOFFS + 1):
            b, e = int(lm.arc_offsets[q]), int(lm.arc_offsets[q + 1])
            j = b + int(np.searchsorted(lm.arc_labels[b:e], c))
            if j < e and int(lm.arc_labels[j]) == c:
                w = F(lm.arc_weight[j])
                g, n = (F(prod * w) if depth else w), int(lm.arc_next[j])
                return (g, n, depth) if with_depth else (g, n)
            if int(lm.backoff[q]) < 0:
                break
            prod = _flush(F(prod * _flush(lm.backoff_weight[q], F)), F)
            q = int(lm.backoff[q])
    return (F(0), -1, depth) if with_depth else (F(0), -1)


def sparse_lm_to_dense(lm):
    """the model expanded through sparse_lm_lookup into the tables of CtcLabelLm: (next int32 [Q, K], weight float32 [Q, K], final);
    next is -1 where the lookup forbids or leaves [0, Q).  For small models: Q K entries.  A row is filled level by level down the
    back-off chain of its state, every entry by the multiplications sparse_lm_lookup does for it, in its order (a valid model:
    sparse_lm_validate)."""
    F = np.float32
    Q, K = len(lm.backoff), lm.classes
    off, lab, arc_next = np.asarray(lm.arc_offsets), np.asarray(lm.arc_labels), np.asarray(lm.arc_next)
    arc_wt = np.asarray(lm.arc_weight, F)
    nxt, wt = np.full((Q, K), -1, np.int32), np.zeros((Q, K), F)
    with np.errstate(all="ignore"):
        for q in range(Q):
            filled, prod, s = np.zeros(K, bool), F(1), q
            for depth in range(SPARSE_MAX_BACKOFFS + 1):
                b, e = int(off[s]), int(off[s + 1])
                new = ~filled[lab[b:e]]
                idx = lab[b:e][new]
                wt[q, idx] = (prod * arc_wt[b:e][new]).astype(F) if depth else arc_wt[b:e][new]
                n = arc_next[b:e][new]
                nxt[q, idx] = np.where((n >= 0) & (n < Q), n, -1)
                filled[idx] = True
                if int(lm.backoff[s]) < 0:
                    break
                prod = _flush(F(prod * _flush(lm.backoff_weight[s])))
                s = int(lm.backoff[s])
    return nxt, wt, (None if lm.final is None else np.asarray(lm.final, F))


def sparse_lm_validate(lm, blank):
    """What klstm_ctc_slm_build makes of the arrays, on the host: (the model as cut, status [8]).  A state is DROPPED -- it loses its
    arcs and keeps its back-off -- for [3] an arc range outside [0, A], or by its first arc at fault: [1] a label outside [0, K), [2]
    the blank, [0] a label not above the one before.  A back-off is CUT to -1 for [4] a target outside [-1, Q) and for [5] a chain of
    more than SPARSE_MAX_BACKOFFS back-offs, cycles included, decided for every state on the range-checked array.  [6] counts the
    states the device stores as a direct row (at least K / 4 arcs): a matter of layout, not of content."""
    K, Q, A = lm.classes, len(lm.backoff), len(lm.arc_labels)
    off, lab = [int(v) for v in lm.arc_offsets], [int(v) for v in lm.arc_labels]
    status = [0] * 8
    ranges = []
    for q in range(Q):
        b, e, why = off[q], off[q + 1], -1
        if b < 0 or e < b or e > A:
            why = 3
        else:
            prev = -1
            for j in range(b, e):
                c = lab[j]
                why = 1 if c < 0 or c >= K else 2 if c == blank else 0 if c <= prev else -1
                if why >= 0:
                    break
                prev = c
        if why >= 0:
            status[why] += 1
            b = e = 0
        ranges.append((b, e))
        if e - b > 0 and (e - b) * 4 >= K:
            status[6] += 1
    raw = []
    for q in range(Q):
        bo = int(lm.backoff[q])
        if bo < -1 or bo >= Q:
            status[4] += 1
            bo = -1
        raw.append(bo)
    cut = list(raw)
    for q in range(Q):
        d, s = 0, raw[q]
        while s >= 0 and d <= SPARSE_MAX_BACKOFFS:
            d, s = d + 1, raw[s]
        if d > SPARSE_MAX_BACKOFFS:
            cut[q] = -1
            status[5] += 1
    offsets, labels, nxt, wt = [0], [], [], []
    for b, e in ranges:
        labels += lab[b:e]
        nxt += [int(v) for v in lm.arc_next[b:e]]
        wt += [np.float32(v) for v in lm.arc_weight[b:e]]
        offsets.append(len(labels))
    out = SparseLm(K, np.asarray(offsets, np.int64), np.asarray(labels, np.int64), np.asarray(nxt, np.int64), np.asarray(wt, np.float32),
                   np.asarray(cut, np.int64), np.asarray(lm.backoff_weight, np.float32), lm.final)
    return out, status


def _sparse_from_states(K, states, arcs_of, bow_of, final_of, order, dtype):
    """states: the histories (tuples; -1 stands for the start of the sequence), states[0] the start; arcs_of(h) -> {label: weight};
    the next state of (h, c) is the longest suffix of h + (c,) that is a state, the back-off of h its longest proper suffix that is"""
    index = {h: i for i, h in enumerate(states)}

    def longest(h):
        while h not in index:
            h = h[1:]
        return index[h]
    offsets, labels, nxt, wt, backoff, bow, fin = [0], [], [], [], [], [], []
    for h in states:
        for c, g in sorted(arcs_of(h).items()):
            labels.append(c); wt.append(g)
            nxt.append(longest((h + (c,))[-(order - 1):] if order > 1 else ()))
        offsets.append(len(labels))
        backoff.append(longest(h[1:]) if h else -1)
        bow.append(bow_of(h) if h else 1.0)
        fin.append(final_of(h))
    depth = max(len(h) for h in states)
    assert depth <= SPARSE_MAX_BACKOFFS, "a back-off chain of %d: orders up to %d" % (depth, SPARSE_MAX_BACKOFFS + 1)
    return SparseLm(K, np.asarray(offsets, np.int32), np.asarray(labels, np.int32), np.asarray(nxt, np.int32), np.asarray(wt, dtype),
                    np.asarray(backoff, np.int32), np.asarray(bow, dtype), np.asarray(fin, dtype))


def _ordered_states(histories, order):
    """the start history first ((-1,), or () for a unigram), then the empty history, then the others by length and content"""
    start = (-1,) if order > 1 else ()
    rest = sorted(set(histories) - {start, ()}, key=lambda h: (len(h), h))
    return [start] + ([()] if order > 1 else []) + rest


def arpa_label_lm(path_or_text, symbols, K, blank, alpha=1.0, beta=0.0):
    """Reads a back-off n-gram in ARPA format (a path, or the text itself: it begins with a backslash section or holds a newline)
    into a SparseLm.  symbols: token -> class (a dict, or a sequence whose index is the class); n-grams with a token that maps to no
    class are skipped, as are those with <s> anywhere but first or </s> anywhere but last.  States are the histories (every listed
    n-gram below the highest order, every context), the <s> history is state 0; the next state is the longest suffix of history +
    label that is a state; arc weight 10^(alpha logp) e^beta, back-off weight 10^(alpha logbow) (0 where none is given), final =
    P(</s> | history)^alpha with back-off applied, in float64.  Orders up to 9."""
    text = path_or_text
    if "\n" not in text and not text.lstrip().startswith("\\"):
        with open(path_or_text) as fh:
            text = fh.read()
    if not isinstance(symbols, dict):
        symbols = {tok: i for i, tok in enumerate(symbols) if tok is not None}
    logp, logbow, order, n = {}, {}, 0, 0
    for line in text.splitlines():
        f = line.split()
        if not f:
            continue
        if f[0].startswith("\\"):
            n = int(f[0][1:f[0].index("-")]) if f[0].endswith("-grams:") else 0
            order = max(order, n)
            continue
        if n == 0 or len(f) < n + 1:
            continue
        gram, ok = [], True
        for i, tok in enumerate(f[1:n + 1]):
            if tok == "<s>":
                ok &= i == 0
                gram.append(-1)
            elif tok == "</s>":
                ok &= i == n - 1
                gram.append(-2)
            else:
                c = symbols.get(tok)
                ok &= c is not None and 0 <= c < K and c != blank
                gram.append(c)
        if not ok:
            continue
        gram = tuple(gram)
        logp[gram] = float(f[0])
        if len(f) > n + 1:
            logbow[gram] = float(f[n + 1])
    assert 1 <= order <= SPARSE_MAX_BACKOFFS + 1, "orders 1 to %d" % (SPARSE_MAX_BACKOFFS + 1)
    hist = {()}
    for gram in logp:
        hist.add(gram[:-1])
        if len(gram) < order and gram[-1] != -2:
            hist.add(gram)
    states = _ordered_states(hist, order)

    by_hist = {}
    for gram, lp in logp.items():
        if gram[-1] >= 0:
            by_hist.setdefault(gram[:-1], {})[gram[-1]] = 10.0 ** (alpha * lp) * math.exp(beta)

    def end_log(h):
        acc = 0.0
        while True:
            if h + (-2,) in logp:
                return acc + logp[h + (-2,)]
            if not h:
                return -math.inf
            acc += logbow.get(h, 0.0)
            h = h[1:]

    def final_of(h):
        lp = end_log(h)
        return 10.0 ** (alpha * lp) if lp > -math.inf else 0.0
    return _sparse_from_states(K, states, lambda h: by_hist.get(h, {}), lambda h: 10.0 ** (alpha * logbow.get(h, 0.0)), final_of, order,
                               np.float32)


def backoff_ngram_label_lm(sequences, K, blank, order=3, discount=0.75, alpha=1.0, beta=0.0, dtype=np.float32):
    """An absolute-discounting back-off n-gram over label sequences (lists of classes other than the blank), order 1 to 9, as a
    SparseLm.  Events are the K - 1 labels and the end of the sequence; histories are the last order - 1 tokens, the start of the
    sequence among them.  For a history h with n(h) events, d(h) of them distinct: P(w | h) = (n(h, w) - discount) / n(h) for a seen
    event, and bow(h) P(w | h') for an unseen one, h' being h without its oldest token and bow(h) = discount d(h) / n(h) over the mass
    h' gives to the events unseen in h (a history that has seen all K events is not discounted).  The empty history spreads its left-over mass evenly over all K events, so every label has an
    arc there and every distribution sums to 1.  Arc weight P^alpha e^beta, back-off weight bow^alpha, final P(end | h)^alpha with
    back-off applied; everything is computed in float64 and cast to `dtype` at the end."""
    assert 1 <= order <= SPARSE_MAX_BACKOFFS + 1 and 0.0 < discount < 1.0
    END = K                                                  # the end of the sequence as one more event
    counts = {}
    for seq in sequences:
        ctx = [-1]
        for w in [int(c) for c in seq] + [END]:
            assert w == END or (0 <= w < K and w != blank), "labels are classes other than the blank"
            for k in range(min(order - 1, len(ctx)) + 1):
                h = tuple(ctx[len(ctx) - k:])
                row = counts.setdefault(h, {})
                row[w] = row.get(w, 0) + 1
            ctx.append(w)
    counts.setdefault((), {})
    if order > 1:
        counts.setdefault((-1,), {})
    states = _ordered_states(counts.keys(), order)
    full, seen_p, bows = {}, {}, {}
    for h in sorted(states, key=len):                        # a history after the one it backs off to
        row = counts[h]
        n = float(sum(row.values()))
        p = np.zeros(K + 1, np.float64)
        if not h:
            if n > 0:
                for w, cnt in row.items():
                    p[w] = (cnt - discount) / n
                left = discount * len(row) / n
            else:
                left = 1.0
            share = np.full(K + 1, left / K)
            share[blank] = 0.0
            p = p + share
            seen_p[h], bows[h] = {w: p[w] for w in range(K + 1) if w != blank}, 1.0
        else:
            low = full[h[1:]]
            if len(row) == K:                                # every event seen: nothing to back off to, so nothing is discounted
                sp, bow = {w: cnt / n for w, cnt in row.items()}, 0.0
            elif n > 0:
                sp = {w: (cnt - discount) / n for w, cnt in row.items()}
                bow = discount * len(row) / n / (1.0 - sum(low[w] for w in sp))
            else:
                sp, bow = {}, 1.0
            p = bow * low
            for w, v in sp.items():
                p[w] = v
            seen_p[h], bows[h] = sp, bow
        full[h] = p
    ebeta = math.exp(beta)

    def arcs_of(h):
        return {w: v ** alpha * ebeta for w, v in seen_p[h].items() if w != END}
    return _sparse_from_states(K, states, arcs_of, lambda h: bows[h] ** alpha, lambda h: full[h][END] ** alpha, order, dtype)


# ------------------------------------------------------------------------------------------------------------------------------------
# Words for the second pass (klstm_ctc_nbest_rescore of include/klstm.h; ctc.ctc_nbest_rescore, ctc.CtcWordTable):
# a word is a run of tokens between separators, known on the device by the 64-bit hash the beam search knows its prefixes by.  A word
# model is a SparseLm over V classes, one per word of the vocabulary, one for unknown words if wanted, and one reserved: the `blank`
# it is built with, which no word ever maps to.
# ------------------------------------------------------------------------------------------------------------------------------------
_WORD_H0, _WORD_HMUL, _M64 = 0x243F6A8885A308D3, 0x9E3779B97F4A7C15, (1 << 64) - 1      # KLSTM_CTC_HASH_START, KLSTM_CTC_HASH_MUL of include/klstm.h


def word_key(tokens):
    """the key of a word: h <- x ^ (x >> 29) with x = (h ^ (token + 1)) * 0x9E3779B97F4A7C15 mod 2^64, folded over its tokens"""
    h = _WORD_H0
    for c in tokens:
        x = ((h ^ ((int(c) + 1) & 0xFFFFFFFF)) * _WORD_HMUL) & _M64
        h = x ^ (x >> 29)
    return h


def split_words(tokens, separator):
    """-> the words: the maximal runs of tokens other than the separator, none empty (the device's rule: csrc/klstm_ctc_nbest.h)"""
    words, word = [], []
    for t in [int(c) for c in tokens] + [separator]:
        if t != separator:
            word.append(t)
        elif word:
            words.append(word)
            word = []
    return words


def word_table(words, separator, ids=None):
    """words: the vocabulary, each word a non-empty list of token classes other than the separator; ids: the class of each in the word
    model (None: its position).  -> (keys uint64 [W] ascending, ids int32 [W] in that order), the arrays of CtcWordTable.  Raises
    ValueError where two different words share a key, or one word is listed twice."""
    ids = list(range(len(words))) if ids is None else [int(i) for i in ids]
    assert len(ids) == len(words)
    seen = {}
    for w, i in zip(words, ids):
        w = tuple(int(c) for c in w)
        assert len(w) > 0 and separator not in w and min(w) >= 0, "a word is a non-empty run of classes other than the separator"
        k = word_key(w)
        if k in seen:
            raise ValueError("the words %r and %r share the key %#x" % (list(seen[k][0]), list(w), k) if seen[k][0] != w
                             else "the word %r is listed twice" % (list(w),))
        seen[k] = (w, i)
    keys = sorted(seen)
    return np.asarray(keys, np.uint64), np.asarray([seen[k][1] for k in keys], np.int32)


def word_sequences(label_seqs, table, separator, unk_id):
    """label sequences (tokens with separators) -> the sequences of word classes a word model is trained on
    (backoff_ngram_label_lm(..., K=V, blank=reserved)).  table: what word_table() returned.  A word that is not in the table takes
    unk_id; with unk_id < 0 the sequence is left out, as the rescoring forbids such an entry."""
    keys, ids = table
    index = {int(k): int(i) for k, i in zip(keys, ids)}
    out = []
    for seq in label_seqs:
        row = [index.get(word_key(word), unk_id) for word in split_words(seq, separator)]
        if all(i >= 0 for i in row):
            out.append(row)
    return out


def dense_lm_to_sparse(next, weight, final=None, blank=None):
    """the dense tables of CtcLabelLm (ngram_label_lm / lexicon_label_lm) as a SparseLm without back-offs, so that a first pass run with
    them can be taken out by ctc_nbest_rescore(sub=...): state q keeps an arc for every class c with next[q, c] in [0, Q) and
    weight[q, c] > 0 -- what the dense search does not forbid -- and a class without an arc is forbidden.  blank: its column is left
    out whatever it holds."""
    nxt, wt = np.asarray(next), np.asarray(weight, np.float32)
    Q, K = nxt.shape
    keep = (nxt >= 0) & (nxt < Q) & (wt > 0)
    if blank is not None:
        keep[:, blank] = False
    q_idx, c_idx = np.nonzero(keep)                          # row by row, classes ascending
    offsets = np.zeros(Q + 1, np.int32)
    offsets[1:] = np.cumsum(keep.sum(1))
    return SparseLm(K, offsets, c_idx.astype(np.int32), nxt[q_idx, c_idx].astype(np.int32), wt[q_idx, c_idx], np.full(Q, -1, np.int32),
                    np.ones(Q, np.float32), None if final is None else np.asarray(final, np.float32))
