"""The twin of klstm_ctc_beam_decode_slm (include/klstm.h; tests/test_ctc_beam_slm.py, tests/test_ctc_beam_slm_gpu.py), host only.  No
second search is written: the twin is beam_twin_lm of tests/ctc_beam_lm_ref.py, fed either with the expansion of the sparse model
(sparse_lm_to_dense of kaldi-lstm_amd/lm.py) or, for models too large to expand, with table objects that answer [q, c] through
sparse_lm_lookup -- the definition of a lookup, which the device reproduces bit for bit.  The lazy tables also count how far the
lookups backed off.  Below them: the models and the cases the two test files share."""
import collections

import numpy as np

from tests import ctc_beam_lm_ref as L
from tests import ctc_beam_ref as Bm
from tests.ctc_beam_ref import candidates_all, emissions

STRONG = np.float32(2.0 ** -30)      # a factor and an emission at or above it: their product is at or above 2^-60, so f > 0


def lm_module():
    import kaldi_lstm_amd as k
    return k.lm


class LazyTables:
    """next and weight tables of a sparse model that answer [q, c] through sparse_lm_lookup (cached).  depth[d]: the lookups that
    backed off d times and gave a factor >= 2^-30 with a next state inside [0, Q), each (q, c) counted once; reads[d]: every read
    of the weight table, that is every extension the search built, by the back-offs its lookup took"""

    def __init__(self, model):
        self.model, self.Q, self.K = model, len(model.backoff), model.classes
        self.cache, self.depth, self.reads = {}, collections.Counter(), collections.Counter()
        self.lookup = lm_module().sparse_lm_lookup
        self.nxt, self.wt = _View(self, 1), _View(self, 0)

    def get(self, q, c):
        key = (int(q), int(c))
        hit = self.cache.get(key)
        if hit is None:
            g, n, d = self.lookup(self.model, key[0], key[1], with_depth=True)
            g = emissions(np.asarray([g], np.float32))[0]             # flushed, as lm_tables flushes a dense table
            hit = self.cache[key] = (g, n, d)
            if g >= STRONG and 0 <= n < self.Q:
                self.depth[d] += 1
        return hit


class _View:
    def __init__(self, tables, field):
        self.tables, self.field, self.shape = tables, field, (tables.Q, tables.K)

    def __getitem__(self, qc):
        hit = self.tables.get(*qc)
        if self.field == 0:
            self.tables.reads[hit[2]] += 1
        return hit[self.field]


def final_of(model, final="model"):
    return model.final if isinstance(final, str) else final


def beam_twin_slm(y, lens, blank, beam, cands, nbest, model, final="model", w=None, refs=None, lazy=False, stats=None):
    """beam_twin_lm on the sparse model.  lazy: through LazyTables (returned as the second value) instead of the expansion"""
    fin = final_of(model, final)
    if not lazy:
        nxt, wt, _ = lm_module().sparse_lm_to_dense(model)
        return L.beam_twin_lm(y, lens, blank, beam, cands, nbest, (nxt, wt, fin), w=w, refs=refs, stats=stats), None
    tabs = LazyTables(model)
    flushed = emissions(np.asarray(fin, np.float32)) if fin is not None else None
    saved = L.lm_tables
    L.lm_tables = lambda lm: (tabs.nxt, tabs.wt, flushed)            # the one thing beam_twin_lm does with its `lm`
    try:
        return L.beam_twin_lm(y, lens, blank, beam, cands, nbest, None, w=w, refs=refs, stats=stats), tabs
    finally:
        L.lm_tables = saved


def weakest_candidate(y, lens, blank, cands, w=None):
    """the smallest emission among the candidates of the valid frames"""
    y = np.asarray(y, np.float32)
    low = np.float32(np.inf)
    for s, n in enumerate(lens):
        if 0 < n <= y.shape[0]:
            e = emissions(y[:n, s], w)
            for t, cand in enumerate(candidates_all(e, blank, cands)):
                for c in cand:
                    low = min(low, e[t, c])
    return low


# ---------------------------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------------------------
def markov_sequences(rng, K, blank, count, longest, peak=0.15):
    """label sequences from a random second-order chain with peaked rows, so that long histories come back"""
    labels = [c for c in range(K) if c != blank]
    n = len(labels)
    rows = rng.dirichlet([peak] * n, size=n * n)
    out = []
    for _ in range(count):
        a, b, seq = rng.randint(n), rng.randint(n), []
        for _ in range(rng.randint(1, longest + 1)):
            a, b = b, int(rng.choice(n, p=rows[a * n + b]))
            seq.append(labels[b])
        out.append(seq)
    return out


def chain_sequences(rng, K, blank, count, longest, peak=0.02):
    """label sequences from a random first-order chain with peaked rows: cheap at a large K"""
    labels = [c for c in range(K) if c != blank]
    n = len(labels)
    rows = rng.dirichlet([peak] * n, size=n)
    out = []
    for _ in range(count):
        b, seq = rng.randint(n), []
        for _ in range(rng.randint(2, longest + 1)):
            b = int(rng.choice(n, p=rows[b]))
            seq.append(labels[b])
        out.append(seq)
    return out


def explicit_model(rng, K, blank, Q, zero=0.2, final=True):
    """no back-off at all: every state has an arc for every label"""
    lm = lm_module()
    labels = np.asarray([c for c in range(K) if c != blank], np.int32)
    n = len(labels)
    wt = np.exp(rng.randn(Q * n)).astype(np.float32)
    wt[rng.rand(Q * n) < zero] = 0.0
    return lm.SparseLm(K, np.arange(Q + 1, dtype=np.int32) * n, np.tile(labels, Q), rng.randint(0, Q, Q * n).astype(np.int32), wt,
                       np.full(Q, -1, np.int32), np.ones(Q, np.float32), (0.05 + rng.rand(Q)).astype(np.float32) if final else None)


def counted_model(seed, K, blank, order, count=40, longest=12, alpha=0.8, beta=0.4):
    rng = np.random.RandomState(9000 + seed)
    return lm_module().backoff_ngram_label_lm(markov_sequences(rng, K, blank, count, longest), K, blank, order=order, alpha=alpha, beta=beta)


def without_final(model):
    return model._replace(final=None)


# ---------------------------------------------------------------------------------------------------------------------------------
# the back-off coverage cases: seeds picked on the CPU (tests/test_ctc_beam_slm.py holds them to the condition) so that on the twin
# lookups of every back-off depth 0 to 4 occur among the extensions with f > 0 and the LM changes the 1-best of some stream
# ---------------------------------------------------------------------------------------------------------------------------------
COVERAGE_SEEDS = (1, 2)
COVERAGE_SHAPE = dict(S=3, T=40, K=12, B=8, C=5, N=3, blank=0, order=5)


def coverage_case(seed):
    from tests.test_ctc_beam import softmax_rows
    sh = COVERAGE_SHAPE
    rng = np.random.RandomState(500 + seed)
    y = softmax_rows(rng, sh["T"], sh["S"], sh["K"])
    lens = [sh["T"], 23, 9]
    return y, lens, counted_model(seed, sh["K"], sh["blank"], sh["order"])


def coverage_findings(y, lens, model, tw, tabs):
    """(the depths 0 to 4 that are missing among the strong lookups, the streams whose 1-best the LM changed, the weakest candidate)"""
    sh = COVERAGE_SHAPE
    plain = Bm.beam_twin(y, lens, sh["blank"], sh["B"], sh["C"], sh["N"])
    changed = [s for s in range(len(lens)) if plain["hyp"][s][:1] != tw["hyp"][s][:1]]
    return [d for d in range(5) if tabs.depth[d] == 0], changed, weakest_candidate(y, lens, sh["blank"], sh["C"])


# ---------------------------------------------------------------------------------------------------------------------------------
# models the build must cut: name -> (the arrays as given, the status counts klstm.h specifies for them)
# ---------------------------------------------------------------------------------------------------------------------------------
BROKEN_K, BROKEN_BLANK = 8, 3
IMAX, IMIN = 2 ** 31 - 1, -2 ** 31


def chain_model(links):
    """states 0 .. links: state q backs off to q + 1, the last to nothing and alone has an arc for every label (to state 1); state 0
    has arcs for the first two labels.  From state 0 a chain of `links` back-offs"""
    lm = lm_module()
    K, blank, Q = BROKEN_K, BROKEN_BLANK, links + 1
    labels = [c for c in range(K) if c != blank]
    off = [0, 2] + [2] * (Q - 2) + [2 + len(labels)]
    lab = labels[:2] + labels
    wt = np.asarray([0.5, 0.25] + [0.1 + 0.1 * i for i in range(len(labels))], np.float32)
    return lm.SparseLm(K, np.asarray(off, np.int64), np.asarray(lab, np.int64), np.ones(len(lab), np.int64), wt,
                       np.asarray(list(range(1, Q)) + [-1], np.int64), np.full(Q, 0.9, np.float32), np.linspace(0.2, 1.0, Q).astype(np.float32))


def broken_models():
    base = counted_model(3, BROKEN_K, BROKEN_BLANK, 3, count=30, longest=10)
    wide = lambda m: m._replace(arc_offsets=m.arc_offsets.astype(np.int64), arc_labels=m.arc_labels.astype(np.int64),      # noqa: E731
                                arc_next=m.arc_next.astype(np.int64), backoff=m.backoff.astype(np.int64))
    base = wide(base)
    off = base.arc_offsets
    deg = np.diff(off)
    two = [q for q in range(2, len(deg)) if deg[q] >= 2]            # states with two arcs or more, the start and the empty history aside
    top = [q for q in range(len(deg)) if q not in set(base.backoff.tolist())][-2:]         # nobody backs off to these
    out = {}
    m = wide(base); q = two[0]
    m.arc_labels[[off[q], off[q] + 1]] = m.arc_labels[[off[q] + 1, off[q]]]
    out["unsorted"] = (m, [1, 0, 0, 0, 0, 0])
    m = wide(base)
    m.arc_labels[off[two[1]] + 1] = m.arc_labels[off[two[1]]]        # equal labels are not ascending either
    out["repeated"] = (m, [1, 0, 0, 0, 0, 0])
    m = wide(base)
    m.arc_labels[off[two[0]]] = BROKEN_BLANK
    out["blank arc"] = (m, [0, 0, 1, 0, 0, 0])
    m = wide(base)
    m.arc_labels[off[two[0]]], m.arc_labels[off[two[1]] + 1] = IMAX, IMIN
    m.backoff[two[2]], m.backoff[two[3]] = IMAX, IMIN
    m.arc_next[off[1]], m.arc_next[off[1] + 1], m.arc_next[off[0]] = IMAX, IMIN, len(deg)
    out["extremes"] = (m, [0, 2, 0, 0, 2, 0])
    m = wide(base)
    m.arc_offsets[two[0] + 1] = IMAX                                 # the range of that state and of the one behind it
    out["offsets"] = (m, [0, 0, 0, 2, 0, 0])
    m = wide(base)
    m.backoff[top[0]], m.backoff[top[1]] = top[1], top[0]
    out["cycle"] = (m, [0, 0, 0, 0, 0, 2])
    out["chain of 8"] = (chain_model(8), [0, 0, 0, 0, 0, 0])
    out["chain of 9"] = (chain_model(9), [0, 0, 0, 0, 0, 1])
    return out
