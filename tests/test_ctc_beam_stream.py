"""The streaming CTC prefix beam search, host side (no GPU): its numpy twin (tests/ctc_beam_stream_ref.py) against the whole-utterance
twins (tests/ctc_beam_ref.py, tests/ctc_beam_lm_ref.py) under random chunkings, the stable prefix as a property of whole runs and on
a hand-built case, the C-ABI's host-side answers, and the refusals of the C++ driver (tests/cpp/ctc_beam_stream_test.cpp)."""
import os
import subprocess

import numpy as np
import pytest

from tests import cpp_driver
from tests import ctc_beam_lm_ref as L
from tests import ctc_beam_ref as Bm
from tests import ctc_beam_stream_ref as R
from tests.test_ctc_beam import softmax_rows
from tests.test_ctc_beam_lm import bigram_next

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_ctc_beam_stream_driver():
    return cpp_driver.build("ctc_beam_stream_test", headers=cpp_driver.HEADERS + ("klstm_scorer.hpp",))


def run_driver(*args):
    return cpp_driver.run("ctc_beam_stream_test", *args, headers=cpp_driver.HEADERS + ("klstm_scorer.hpp",))


def bits(v):
    return [int(np.float32(x).view(np.int32)) for x in v]


def random_bigram(rng, K, zero=0.2, final=True):
    wt = np.exp(rng.randn(K + 1, K)).astype(np.float32)
    wt[rng.rand(K + 1, K) < zero] = 0.0
    return bigram_next(K), wt, ((0.05 + rng.rand(K + 1)).astype(np.float32) if final else None)


def random_chunks(rng, n, longest):
    """a split of n frames into chunks of 1 .. longest frames"""
    out = []
    while sum(out) < n:
        out.append(int(min(rng.randint(1, longest + 1), n - sum(out))))
    return out


def whole_twin(y, lens, blank, B, C, N, lm, final):
    if lm is None:
        return Bm.beam_twin(y, lens, blank, B, C, N)
    return L.beam_twin_lm(y, lens, blank, B, C, N, (lm[0], lm[1], lm[2] if final else None))


def feed(tw, y, plan, call, done):
    """the chunk [T, S, K] and the lens of call number `call` of a per-stream plan (lists of chunk lengths); done: frames consumed.
    Rows that must not be read are NaN."""
    S, K = y.shape[1], y.shape[2]
    lens = [plan[s][call] if call < len(plan[s]) else 0 for s in range(S)]
    T = max(max(lens), 1)
    chunk = np.full((T, S, K), np.nan, np.float32)
    for s in range(S):
        chunk[:lens[s], s] = y[done[s]:done[s] + lens[s], s]
    tw.step(chunk, lens)
    return [done[s] + lens[s] for s in range(S)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the feature exists (fails on a tree without it)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_library_and_package_carry_the_stream_decoder():
    import inspect
    import kaldi_lstm_amd as k
    lib = k.load_library()
    for name in ("klstm_ctc_beam_stream_state_bytes", "klstm_ctc_beam_stream_workspace_bytes", "klstm_ctc_beam_stream_step",
                 "klstm_ctc_beam_stream_emit"):
        assert hasattr(lib, name)
    assert inspect.isclass(k.CtcBeamStream) and {"step", "emit"} <= set(dir(k.CtcBeamStream))
    with open(os.path.join(ROOT, "include", "klstm_nnet.hpp")) as fh:
        assert "class CtcStreamDecoder" in fh.read()
    with open(os.path.join(ROOT, "include", "klstm_scorer.hpp")) as fh:
        hpp = fh.read()
    assert "ForEachChunk" in hpp and "DecodeCtcStreaming" in hpp


# ---------------------------------------------------------------------------------------------------------------------------------
# any chunking: the bits of the whole-utterance twins, at the end and after every call
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_lm", [False, True])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_chunkings_equal_the_whole_utterance_twin(seed, with_lm):
    rng = np.random.RandomState(500 + seed)
    S, T, K, B, C, N = 3, 36, 9, (4, 8, 6)[seed], (3, 5, 8)[seed], (4, 3, 6)[seed]
    blank = (0, K - 1, 4)[seed]
    lens = [T, int(rng.randint(2, T)), 1]
    y = softmax_rows(rng, T, S, K)
    lm = random_bigram(rng, K) if with_lm else None
    plan = [random_chunks(rng, lens[s], 9) for s in range(S)]
    tw = R.BeamStreamTwin(S, K, T, blank, B, C, lm=lm)
    done = [0] * S
    for call in range(max(len(p) for p in plan)):
        done = feed(tw, y, plan, call, done)
        for mode in ((1, 2) if with_lm else (1,)):
            got = tw.emit([mode] * S, N)
            want = whole_twin(y, done, blank, B, C, N, lm, mode == 2)
            assert got["hyp"] == want["hyp"] and got["nbest_count"] == want["nbest_count"], (call, mode)
            assert [bits(v) for v in got["score"]] == [bits(v) for v in want["score"]], (call, mode)
            assert got["frames"] == done
    assert done == lens


def test_streams_restart_idle_and_overflow_without_leaking():
    """a second utterance started in a stream while its neighbour is in mid-utterance; an idle call in mid-utterance, with start set;
    one frame beyond max_frames: rejected, the state as it was"""
    rng = np.random.RandomState(77)
    S, K, B, C, N, F = 2, 7, 6, 4, 3, 20
    ya, yb, yc = (softmax_rows(rng, F, 1, K) for _ in range(3))
    tw = R.BeamStreamTwin(S, K, F, 0, B, C)
    nan = np.full((8, 1, K), np.nan, np.float32)
    tw.step(np.concatenate([ya[:8], yb[:8]], 1), [8, 8])
    tw.step(np.concatenate([ya[8:16], nan], 1), [8, 0], start=[0, 1])                # stream 1 idle, start ignored
    tw.step(np.concatenate([yc[:8], yb[8:16]], 1), [8, 8], start=[1, 0])             # a new utterance in stream 0
    got = tw.emit([1, 1], N)
    want = Bm.beam_twin(np.concatenate([yc[:8], yb[:16]], 1) if False else np.stack([np.pad(yc[:8, 0], ((0, 8), (0, 0))), yb[:16, 0]], 1),
                        [8, 16], 0, B, C, N)
    assert got["hyp"] == want["hyp"] and [bits(v) for v in got["score"]] == [bits(v) for v in want["score"]] and got["frames"] == [8, 16]
    tw.step(np.concatenate([nan[:4], yb[16:20]], 1), [0, 4])                          # max_frames exactly reached
    before = tw.emit([1, 1], N)
    assert before["frames"] == [8, 20]
    tw.step(np.concatenate([nan[:1], yb[:1]], 1), [0, 1])                             # one more: rejected
    after = tw.emit([1, 1], N)
    assert after["frames"] == [8, -21]
    assert after["hyp"] == before["hyp"] and [bits(v) for v in after["score"]] == [bits(v) for v in before["score"]]
    assert tw.emit([0, 2], N)["nbest_count"][0] == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# the stable prefix
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_lm", [False, True])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_stable_prefix_begins_every_later_hypothesis(seed, with_lm):
    """after every frame: the first stable_len tokens of the 1-best begin EVERY hypothesis of EVERY later emit (full lists, both modes)"""
    rng = np.random.RandomState(900 + seed)
    K, T, B, C = (5, 9, 12, 7)[seed], 50, (4, 8, 3, 16)[seed], (3, 4, 6, 6)[seed]
    y = softmax_rows(rng, T, 1, K, scale=(2.0, 3.0, 1.0, 4.0)[seed])
    lm = random_bigram(rng, K, zero=0.3) if with_lm else None
    tw = R.BeamStreamTwin(1, K, T, 0, B, C, lm=lm)
    pinned, grew = [], 0
    for t in range(T):
        tw.step(y[t:t + 1], [1])
        for mode in ((1, 2) if with_lm else (1,)):
            e = tw.emit([mode], B)
            for n, head in pinned:
                for h in e["hyp"][0]:
                    assert h[:n] == head, (t, n)
        e = tw.emit([1], B)
        n = e["stable_len"][0]
        assert n <= min(len(h) for h in e["hyp"][0])
        grew += bool(pinned) and n > pinned[-1][0]
        pinned.append((n, e["hyp"][0][0][:n]))
    assert grew > 0 and pinned[-1][0] > 0                           # not vacuous: the prefix does become stable


def returning_prefix_case():
    """K = 3, beam 2, one candidate a frame, a bigram that forbids label 2 at the start: "1" enters the beam (node A), is pushed out by
    its own extension "1 2" while the empty prefix stays, and comes back as a NEW extension of the empty prefix (node A').  The beam
    then holds "1 2 1" (through A) and "1" (A'): one common token, two different nodes for it."""
    y = np.array([[0.5, 0.4, 0.1], [0.1, 0.0, 0.9], [0.05, 0.9, 0.05]], np.float32).reshape(3, 1, 3)
    wt = np.ones((4, 3), np.float32)
    wt[0, 2] = 0.0
    return y, (bigram_next(3), wt, None), 2, 1


def test_stable_len_is_exact_when_a_prefix_left_the_beam_and_came_back():
    y, lm, B, C = returning_prefix_case()
    tw = R.BeamStreamTwin(1, 3, 3, 0, B, C, lm=lm)
    tw.step(y, [3])
    z = tw.z[0]
    e = tw.emit([1], B)
    assert e["hyp"][0] == [[1, 2, 1], [1]]
    first = [nd for nd, _, _ in z.beam]
    up = first[0]
    while z.ln[up] > 1:
        up = z.par[up]
    assert up != first[1] and z.tok[up] == z.tok[first[1]] == 1     # the same prefix "1" under two nodes
    assert e["stable_len"] == [1]                                   # a walk that stops at unequal nodes would say 0


def test_stable_len_of_a_dead_beam_is_its_first_entry():
    rng = np.random.RandomState(5)
    y = softmax_rows(rng, 6, 1, 5)
    y[4] = 0.0
    tw = R.BeamStreamTwin(1, 5, 6, 0, 4, 3)
    tw.step(y, [6])
    e = tw.emit([1], 4)
    want = Bm.beam_twin(y, [6], 0, 4, 3, 4)
    assert e["nbest_count"] == [1] and e["hyp"] == want["hyp"] and e["score"][0][0] == -np.inf
    assert e["stable_len"] == [len(e["hyp"][0][0])]


# ---------------------------------------------------------------------------------------------------------------------------------
# the C-ABI's host-side answers and the C++ driver's refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_sizes_and_limits_of_the_c_abi():
    import kaldi_lstm_amd as k
    lib = k.load_library()
    state = lib.klstm_ctc_beam_stream_state_bytes
    assert state(100, 4, 16) > 0 and state(100, 4, 16) % 256 == 0
    assert state(200, 4, 16) - state(100, 4, 16) >= 4 * 100 * 16 * 8              # the tree: 8 bytes per frame and beam entry
    assert state(100, 8, 16) == 2 * state(100, 4, 16)
    for bad in ((0, 4, 16), (100, 0, 16), (100, 33, 16), (100, 4, 0), (100, 4, 65), ((1 << 31) // 64, 4, 64)):
        assert state(*bad) == 0 and b"klstm_ctc_beam_stream_state_bytes" in lib.klstm_last_error()
    assert state((1 << 31) // 64 - 1, 1, 64) > 0                                   # frames * beam + 1 < 2^31: the last that fits
    ws = lib.klstm_ctc_beam_stream_workspace_bytes
    assert ws(50, 32, 8, 4) > ws(20, 32, 8, 4) > 0
    for bad in ((0, 4, 8, 1), (2048, 32, 8, 1), (10, 33, 8, 1), (10, 4, 33, 1), (10, 4, 8, 0), (10, 4, 8, 65)):
        assert ws(*bad) == 0
    n = None
    # sizes are judged before any pointer is looked at: KLSTM_ERR_SHAPE (2) beyond the limits, then KLSTM_ERR_ARG (1) for the nulls
    def step(T=10, S=4, K=8, B=4, C=4, Q=0, frames=100):
        return lib.klstm_ctc_beam_stream_step(n, T, S, K, K, n, n, 0, n, B, C, Q, n, n, n, 0, frames, n, 0, n)

    def emit(S=4, K=8, B=4, N=1, Q=0, frames=100, stride=100):
        return lib.klstm_ctc_beam_stream_emit(S, K, 0, B, N, n, Q, n, n, 0, frames, n, stride, n, n, n, n, n, n, n, n, n, n, 0, n)
    assert step() == 1 and emit() == 1
    for kw in (dict(S=33), dict(T=16384), dict(K=32769), dict(B=65), dict(C=33), dict(C=8), dict(Q=(1 << 24) // 8 + 1),
               dict(frames=0), dict(frames=(1 << 31) // 4, B=4)):
        assert step(**kw) == 2, kw
    for kw in (dict(S=33), dict(K=32769), dict(B=65), dict(N=5), dict(frames=0), dict(stride=99), dict(Q=(1 << 24) // 8 + 1)):
        assert emit(**kw) == 2, kw


def test_driver_usage_and_refusals():
    """a bidirectional model, beam 0, log scores, more than 32 streams and a state beyond the limits are turned down with a message,
    before any device work (this runs without a GPU)"""
    r = run_driver("refuse")
    assert "refused=1" in r.stdout and "bidirectional" in r.stderr
    u = subprocess.run([build_ctc_beam_stream_driver()], capture_output=True, text=True, timeout=60)
    assert u.returncode == 2 and "usage: ctc_beam_stream_test" in u.stderr
