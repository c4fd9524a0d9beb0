"""The numpy twins of the CTC beam search (tests/ctc_beam_ref.py, ctc_beam_lm_ref.py, ctc_beam_slm_ref.py, ctc_beam_stream_ref.py) pinned
to their own bits, host only: a small seeded set of cases, one sha256 per case over everything the twins return, compared with
tests/golden/ctc_beam_twin_digest.json.  The file is a regression anchor recorded from the twins themselves (tests/golden/README.md),
so that a rewrite of the twins can be told from a change of the definition; what makes the twins RIGHT is checked in
tests/test_ctc_beam.py and tests/test_ctc_beam_lm.py against the float64 textbook search and the exact label probability.
    python -m tests.test_ctc_beam_twin_digest --record        writes the file anew (a deliberate change of the definition says so)
The inputs are made here from RandomState draws, products and quotients alone, so that no other file's helpers and no exp or pow
stand between a seed and its digest.  Scores go in as float32 bit patterns: -inf and the last bit count."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from tests import ctc_beam_lm_ref as L
from tests import ctc_beam_ref as Bm
from tests import ctc_beam_slm_ref as Sl
from tests import ctc_beam_stream_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ctc_beam_twin_digest.json")


def canon(x):
    """ints as ints, float32 as its bits, float64 as its hex, containers as lists and dicts; anything else is an error"""
    if x is None:
        return None
    if isinstance(x, (bool, np.bool_)):
        return int(x)
    if isinstance(x, (int, np.integer)):
        return int(x)
    if isinstance(x, np.float32):
        return {"f32": int(x.view(np.uint32))}
    if isinstance(x, (float, np.float64)):
        return {"f64": float(x).hex()}
    if isinstance(x, dict):
        return {str(k): canon(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [canon(v) for v in x]
    if isinstance(x, np.ndarray):
        return [canon(v) for v in x]
    raise TypeError(type(x))


def digest(x):
    return hashlib.sha256(json.dumps(canon(x), sort_keys=True, separators=(",", ":")).encode()).hexdigest()


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def posteriors(seed, T, S, K):
    """rows that sum to 1, peaked (u^4 over its sum): multiplications and one division per value"""
    u = np.random.RandomState(4100 + seed).rand(T, S, K)
    u = u * u * u * u
    return (u / u.sum(-1, keepdims=True)).astype(np.float32)


def bigram(seed, K, final, forbid=False):
    """Q = K + 1, state 1 + c after label c; a fifth of the weights 0, one below 2^-60 and one above 2^60 (both flushed by the rule);
    final: one weight 0, "zero": all of them (every tf is 0).  forbid: a fifth of `next` outside [0, Q), on either side"""
    rng = np.random.RandomState(4200 + seed)
    Q = K + 1
    nxt = np.tile(1 + np.arange(K, dtype=np.int32), (Q, 1))
    wt = (0.1 + 2.0 * rng.rand(Q, K)).astype(np.float32)
    wt[rng.rand(Q, K) < 0.2] = 0.0
    wt[1, 2], wt[2, 1] = 1e-30, 1e30
    fin = None
    if final:
        fin = (0.05 + rng.rand(Q)).astype(np.float32)
        fin[3] = 0.0
        if final == "zero":
            fin[:] = 0.0
    if forbid:
        bad = rng.rand(Q, K) < 0.2
        nxt[bad] = np.where(rng.rand(Q, K) < 0.5, -1, Q)[bad]
        nxt[0, 1] = 2 ** 31 - 1
    return nxt, wt, fin


def references(seed, S, K, blank, spoil=None):
    """one reference per stream; spoil: that stream's holds the blank, so it is not counted"""
    rng = np.random.RandomState(4300 + seed)
    labels = [c for c in range(K) if c != blank]
    refs = [[labels[i] for i in rng.randint(0, len(labels), rng.randint(1, 9))] for _ in range(S)]
    if spoil is not None:
        refs[spoil][0] = blank
    return refs


def plain_cases():
    """name -> (y, lens, blank, B, C, N, w, refs): the search without a language model"""
    out = {}
    y = posteriors(0, 30, 3, 9)
    out["blank 0, refs"] = (y, [30, 17, 5], 0, 8, 4, 4, None, references(0, 3, 9, 0))
    y = posteriors(1, 24, 3, 10)
    out["blank K - 1, a rejected stream, no refs"] = (y, [24, 25, 12], 9, 16, 8, 5, None, None)
    w = (0.5 + np.random.RandomState(4400).rand(7)).astype(np.float32)
    w[2] = 0.0
    y = posteriors(2, 20, 2, 7)
    out["class weights, a reference that is not counted"] = (y, [20, 11], 3, 6, 6, 6, w, references(2, 2, 7, 3, spoil=1))
    y = posteriors(3, 16, 3, 6)
    y[9, 0] = 0.0                                                    # the beam of stream 0 dies in mid-utterance
    out["a dead beam, an idle and a one-frame stream"] = (y, [16, 0, 1], 0, 4, 3, 3, None, references(3, 3, 6, 0))
    return out


def lm_cases():
    """name -> (y, lens, blank, B, C, N, lm, w, refs): a dense automaton"""
    out = {}
    y = posteriors(10, 28, 3, 8)
    out["no final weights"] = (y, [28, 13, 2], 0, 8, 4, 4, bigram(10, 8, False), None, references(10, 3, 8, 0))
    out["final weights"] = (y, [28, 13, 2], 0, 8, 4, 4, bigram(10, 8, True), None, references(10, 3, 8, 0))
    y = posteriors(11, 22, 2, 9)
    out["forbidden transitions, blank K - 1"] = (y, [22, 22], 8, 12, 5, 6, bigram(11, 9, True, forbid=True), None, None)
    y = posteriors(12, 10, 2, 6)
    out["every final weight 0"] = (y, [10, 4], 0, 4, 3, 3, bigram(12, 6, "zero"), None, references(12, 2, 6, 0))
    return out


def slm_case():
    K, blank = 12, 0
    return posteriors(20, 40, 3, K), [40, 21, 9], blank, 8, 5, 3, Sl.counted_model(1, K, blank, 3), references(20, 3, K, blank)


# ---------------------------------------------------------------------------------------------------------------------------------
# what is hashed
# ---------------------------------------------------------------------------------------------------------------------------------
def whole(tw, stats=None):
    keep = {k: tw[k] for k in ("hyp", "score", "nbest_count", "errors", "totals", "state") if k in tw}
    if stats is not None:
        keep["merges"] = stats.get("merges", 0)
    return keep


def streamed(y, lens, blank, B, C, N, lm, w, chunk):
    """the utterances in calls of `chunk` frames a stream (rows that must not be read are NaN); emit in modes 1 and 2 after every call"""
    T, S, K = y.shape
    lens = [n if 0 < n <= T else 0 for n in lens]
    tw = R.BeamStreamTwin(S, K, T, blank, B, C, w=w, lm=lm)
    done, out = [0] * S, []
    while done != lens:
        take = [min(chunk, lens[s] - done[s]) for s in range(S)]
        part = np.full((max(take), S, K), np.nan, np.float32)
        for s in range(S):
            part[:take[s], s] = y[done[s]:done[s] + take[s], s]
        tw.step(part, take)
        done = [done[s] + take[s] for s in range(S)]
        out += [tw.emit([mode] * S, N) for mode in (1, 2)]
    return out


def restart_and_overflow():
    """stream 0 starts a second utterance by `start` while stream 1 goes on; stream 1 idles with start set, reaches max_frames exactly
    and is turned down one frame later; stream 2 never starts; a skipped stream (mode 0)"""
    S, K, B, C, N, frames = 3, 7, 6, 4, 3, 20
    ya, yb, yc = (posteriors(30 + i, frames, 1, K) for i in range(3))
    nan = np.full((8, 1, K), np.nan, np.float32)
    tw = R.BeamStreamTwin(S, K, frames, 0, B, C, lm=bigram(30, K, True))
    out = []
    for chunk, lens, start in ((np.concatenate([ya[:8], yb[:8], nan], 1), [8, 8, 0], None),
                               (np.concatenate([ya[8:16], nan, nan], 1), [8, 0, 0], [0, 1, 1]),
                               (np.concatenate([yc[:8], yb[8:16], nan], 1), [8, 8, 0], [1, 0, 0]),
                               (np.concatenate([nan[:4], yb[16:20], nan[:4]], 1), [0, 4, 0], None),
                               (np.concatenate([nan[:1], yb[:1], nan[:1]], 1), [0, 1, 0], None)):
        tw.step(chunk, lens, start)
        out += [tw.emit(mode, N) for mode in ([1, 1, 1], [2, 2, 2], [0, 2, 1])]
    return out


def cases():
    """name -> a function that returns what is hashed"""
    out = {}
    for name, (y, lens, blank, B, C, N, w, refs) in plain_cases().items():
        out["plain: " + name] = lambda a=(y, lens, blank, B, C, N), w=w, refs=refs: whole(Bm.beam_twin(*a, w=w, refs=refs))
        for chunk in (1, 7, 40):
            out["stream %d, plain: %s" % (chunk, name)] = lambda a=(y, lens, blank, B, C, N, None, w), c=chunk: streamed(*a, c)
    for name, (y, lens, blank, B, C, N, lm, w, refs) in lm_cases().items():
        def run(a=(y, lens, blank, B, C, N, lm), w=w, refs=refs):
            stats = {}
            return whole(L.beam_twin_lm(*a, w=w, refs=refs, stats=stats), stats)
        out["lm: " + name] = run
        for chunk in (1, 7, 40):
            out["stream %d, lm: %s" % (chunk, name)] = lambda a=(y, lens, blank, B, C, N, lm, w), c=chunk: streamed(*a, c)
    for lazy in (False, True):
        def run(lazy=lazy):
            y, lens, blank, B, C, N, model, refs = slm_case()
            stats = {}
            return whole(Sl.beam_twin_slm(y, lens, blank, B, C, N, model, refs=refs, lazy=lazy, stats=stats)[0], stats)
        out["sparse back-off model, order 3, %s" % ("lazy tables" if lazy else "expanded")] = run
    out["stream: restart by start, idle, overflow, never started, skipped"] = restart_and_overflow
    return out


CASES = cases()


def recorded():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_the_file_lists_exactly_the_cases():
    assert sorted(recorded()) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_twin_bits_are_the_recorded_ones(name):
    assert digest(CASES[name]()) == recorded()[name]


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python -m tests.test_ctc_beam_twin_digest --record")
    with open(GOLDEN, "w") as fh:
        json.dump({name: digest(CASES[name]()) for name in sorted(CASES)}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote %s: %d cases" % (GOLDEN, len(CASES)))
