"""Host helpers that build the tables of a label language model for ctc_beam_decode(lm=CtcLabelLm(...)) (klstm_ctc_beam_decode_lm of
include/klstm.h): a dense deterministic weighted automaton over the K classes.  State 0 is the start; label c leads
from state q to next[q, c] and multiplies the prefix probability by weight[q, c]; final[q] multiplies a hypothesis that ends in q.
numpy only.  Both builders return (next int32 [Q, K], weight float32 [Q, K], final float32 [Q]); the blank's column is never read
(next 0, weight 0).  Composing an n-gram with a lexicon (the product automaton) is the caller's."""
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
