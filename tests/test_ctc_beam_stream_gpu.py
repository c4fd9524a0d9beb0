"""The streaming CTC prefix beam search on the GPU (klstm_ctc_beam_stream_step / _emit; kaldi-lstm_amd/csrc/klstm_ctc_beam.hip
k_ctc_beam_stream, k_ctc_beam_emit).  The pass condition is EQUALITY with k.ctc_beam_decode on the same device for the frames consumed
so far: every integer and the int32 view of the scores -- a resumed search has no rounding of its own, so no tolerance is introduced.
Against the stream twin (tests/ctc_beam_stream_ref.py) the integers are equal and the scores within the existing 2 float32 ulps (the
device's double log)."""
import numpy as np
import pytest

from tests import ctc_beam_stream_ref as R
from tests.test_ctc_beam import softmax_rows
from tests.test_ctc_beam_gpu import make_refs, ragged_lens, to_dev, ulps
from tests.test_ctc_beam_stream import random_bigram, returning_prefix_case

pytestmark = pytest.mark.gpu


class Harness:
    """a CtcBeamStream, what it was fed per stream (the current utterance's rows), and the whole-utterance call on exactly those rows"""

    def __init__(self, S, K, max_frames, blank, B, C, N, w=None, lm=None, window=None):
        import torch
        import kaldi_lstm_amd as k
        self.k, self.torch = k, torch
        self.S, self.K, self.blank, self.B, self.C, self.N, self.window = S, K, blank, B, C, N, window
        self.wd = torch.from_numpy(np.asarray(w, np.float32)).cuda() if w is not None else None
        self.lm = lm
        self.dlm = k.CtcLabelLm(*lm) if lm is not None else None
        self.dlm_nofinal = k.CtcLabelLm(lm[0], lm[1], None) if lm is not None else None
        self.bs = k.CtcBeamStream(S, K, max_frames, blank=blank, beam=B, cands=C, class_weight=self.wd, lm=self.dlm)
        self.hist = [np.zeros((0, K), np.float32) for _ in range(S)]

    def step(self, rows, start=None, count=True):
        """rows: per stream an array [n_s, K] (n_s = 0: idle).  Rows of the chunk that must not be read are NaN."""
        lens = [len(r) for r in rows]
        T = max(max(lens), 1)
        chunk = np.full((T, self.S, self.K), np.nan, np.float32)
        for s, r in enumerate(rows):
            chunk[:len(r), s] = r
        self.bs.step(to_dev(chunk, self.window), lens, start=start)
        for s, r in enumerate(rows):
            if len(r) and count:
                fresh = len(self.hist[s]) == 0 or (start is not None and start[s])
                self.hist[s] = np.array(r, np.float32) if fresh else np.concatenate([self.hist[s], r])

    def whole(self, final=True, refs=None, totals=None):
        lens = [len(h) for h in self.hist]
        T = max(max(lens), 1)
        y = np.full((T, self.S, self.K), np.nan, np.float32)
        for s, h in enumerate(self.hist):
            y[:len(h), s] = h
        lm = (self.dlm if final else self.dlm_nofinal) if self.lm is not None else None
        return self.k.ctc_beam_decode(to_dev(y), lens, blank=self.blank, beam=self.B, cands=self.C, nbest=self.N, class_weight=self.wd,
                                      refs=refs, totals=totals, lm=lm)

    def check(self, mode=2, refs=None):
        """emit with `mode` (one value, or one per stream) equals the whole-utterance call on the rows fed so far"""
        modes = [mode] * self.S if isinstance(mode, int) else list(mode)
        res = self.bs.emit(modes, nbest=self.N, refs=refs)
        for m in sorted(set(modes) - {0}):
            same(res, self.whole(final=(m == 2), refs=refs), [s for s in range(self.S) if modes[s] == m], errors=(m == 2))
        cnt = res.nbest_count.cpu().numpy()
        for s in range(self.S):
            if modes[s] == 0:
                assert cnt[s] == 0
        assert res.frames.cpu().numpy().tolist() == [len(h) for h in self.hist]
        return res


def same(ra, rb, streams=None, errors=True):
    """the lists of the streams agree: counts, lengths, tokens, the bits of the scores, errors"""
    ca, cb = ra.nbest_count.cpu().numpy(), rb.nbest_count.cpu().numpy()
    ha, hb, na, nb = ra.hyp.cpu().numpy(), rb.hyp.cpu().numpy(), ra.hyp_len.cpu().numpy(), rb.hyp_len.cpu().numpy()
    sa, sb = ra.score.cpu().numpy().view(np.int32), rb.score.cpu().numpy().view(np.int32)
    for s in (range(len(ca)) if streams is None else streams):
        assert ca[s] == cb[s], s
        for q in range(ca[s]):
            assert na[s, q] == nb[s, q] and ha[s, q, :na[s, q]].tolist() == hb[s, q, :na[s, q]].tolist(), (s, q)
            assert sa[s, q] == sb[s, q], (s, q)
        if errors and ra.errors is not None and rb.errors is not None:
            assert ra.errors[s].cpu().numpy().tolist() == rb.errors[s].cpu().numpy().tolist(), s


def check_twin(res, tw):
    """against the stream twin's emit: integers equal, scores within 2 ulps"""
    cnt = res.nbest_count.cpu().numpy().tolist()
    assert cnt == tw["nbest_count"] and res.frames.cpu().numpy().tolist() == tw["frames"]
    h, n, sc, st = res.hyp.cpu().numpy(), res.hyp_len.cpu().numpy(), res.score.cpu().numpy(), res.stable_len.cpu().numpy()
    for s in range(len(cnt)):
        for q in range(cnt[s]):
            assert h[s, q, :n[s, q]].tolist() == tw["hyp"][s][q], (s, q)
            assert ulps(sc[s, q], tw["score"][s][q]) <= 2, (s, q, sc[s, q], tw["score"][s][q])
        if tw["stable_len"][s] is not None:
            assert st[s] == tw["stable_len"][s], s


def split(y, lens, sizes):
    """per call the rows of every stream: stream s gets the next sizes(s, call) of its lens[s] frames"""
    S = y.shape[1]
    done, calls = [0] * S, []
    call = 0
    while any(done[s] < lens[s] for s in range(S)):
        rows = []
        for s in range(S):
            n = min(sizes(s, call), lens[s] - done[s])
            rows.append(y[done[s]:done[s] + n, s])
            done[s] += n
        calls.append(rows)
        call += 1
    return calls


# ---------------------------------------------------------------------------------------------------------------------------------
# one chunk size for all streams: every partial result is the whole-utterance call on the first n frames
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1, 7, 20, 50, 120])
def test_every_chunk_size_gives_the_whole_utterance_bits(chunk):
    rng = np.random.RandomState(4120)
    S, T, K, B, C, N = 4, 120, 12, 16, 8, 5
    lens = ragged_lens(rng, S, T)                                   # 120, idle, 1, random
    y = softmax_rows(rng, T, S, K)
    h = Harness(S, K, T, 0, B, C, N)
    tw = R.BeamStreamTwin(S, K, T, 0, B, C) if chunk == 20 else None
    for rows in split(y, lens, lambda s, c: chunk):
        h.step(rows)
        res = h.check(1)
        if tw is not None:
            cl = [len(r) for r in rows]
            ch = np.zeros((max(max(cl), 1), S, K), np.float32)
            for s, r in enumerate(rows):
                ch[:len(r), s] = r
            tw.step(ch, cl)
            check_twin(res, tw.emit([1] * S, N))
    assert [len(x) for x in h.hist] == lens


def test_streams_on_chunkings_of_their_own_idle_calls_and_restarts():
    """every stream its own chunk sizes; stream 2 is idle for a call in mid-utterance (with its start flag set: ignored); stream 1
    starts a second utterance while its neighbours are in mid-utterance, stream 3 a third one: nothing leaks between utterances or
    streams"""
    rng = np.random.RandomState(4121)
    S, K, B, C, N, F = 4, 12, 16, 8, 5, 60
    utt = [softmax_rows(rng, F, 1, K)[:, 0] for _ in range(7)]
    h = Harness(S, K, F, 0, B, C, N)
    e = np.zeros((0, K), np.float32)
    h.step([utt[0][:13], utt[1][:5], utt[2][:9], utt[3][:1]]); h.check(1)
    h.step([utt[0][13:20], utt[1][5:30], e, utt[3][1:2]], start=[0, 0, 1, 0]); h.check(1)      # stream 2 idle in mid-utterance
    h.step([utt[0][20:21], utt[4][:17], utt[2][9:40], utt[5][:3]], start=[0, 1, 0, 1]); h.check(1)   # streams 1 and 3 restart
    h.step([utt[0][21:60], utt[4][17:18], e, utt[6][:11]], start=[0, 0, 0, 1]); h.check(1)
    h.step([e, utt[4][18:60], utt[2][40:60], utt[6][11:60]]); res = h.check(1)
    assert res.frames.cpu().numpy().tolist() == [60, 60, 60, 60]


@pytest.mark.parametrize("B,C,N", [(64, 32, 64), (12, 8, 12)])
def test_the_largest_list(B, C, N):
    """B = 64, C = 32, N = 64: 2112 list entries, 256 threads, BEAM_KPT keys a thread; B = 12, C = 8: 108 entries, 128 threads; chunks
    of 3"""
    rng = np.random.RandomState(4122)
    S, T, K = 1, 40, 48
    y = softmax_rows(rng, T, S, K)
    h = Harness(S, K, T, 0, B, C, N)
    tw = R.BeamStreamTwin(S, K, T, 0, B, C)
    for rows in split(y, [T], lambda s, c: 3):
        h.step(rows)
        res = h.check(1)
        tw.step(rows[0][:, None, :], [len(rows[0])])
    check_twin(res, tw.emit([1], N))


@pytest.mark.parametrize("K,B,C,N", [(2, 1, 1, 1), (9, 1, 4, 1), (9, 6, 1, 3), (2, 4, 1, 4), (9, 7, 8, 7)])
def test_edge_parameters_and_a_boundary_after_the_first_frame(K, B, C, N):
    """B = 1, C = 1, K = 2, C = K - 1, N = B; the first chunk is ONE frame: Bc is still growing when the state is stored"""
    rng = np.random.RandomState(K * 100 + B * 10 + C)
    S, T = 3, 30
    lens = [30, 17, 1]
    y = softmax_rows(rng, T, S, K, scale=1.0)
    h = Harness(S, K, T, K - 1, B, C, N)
    for rows in split(y, lens, lambda s, c: (1, 1, 2, 11)[min(c, 3)]):
        h.step(rows)
        h.check(1)


# ---------------------------------------------------------------------------------------------------------------------------------
# with a label language model: tables in LDS and gathered from global memory, final weights, mode 1 against mode 2
# ---------------------------------------------------------------------------------------------------------------------------------
# lists of 16, 108, 144, 200 and 768 entries: 64, 128 and 256 threads, one key and several keys a thread
@pytest.mark.parametrize("K,B,C", [(29, 16, 8), (12, 4, 3), (12, 12, 8), (12, 40, 4), (12, 64, 11)])
@pytest.mark.parametrize("where", ["resident", "gather"])
def test_language_model_resident_and_gathered(where, K, B, C):
    from tests.test_ctc_beam_lm_gpu import pad_states, resident
    rng = np.random.RandomState(4123)
    S, T, N = 3, 40, min(B, 6)
    lens = [40, 23, 1]
    y = softmax_rows(rng, T, S, K)
    lm = random_bigram(rng, K)
    if where == "gather":                                           # padded with unreachable states until the tables leave LDS
        lo, hi = K + 1, (1 << 24) // K
        assert resident(lo, K, B, C) and not resident(hi, K, B, C)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if resident(mid, K, B, C) else (lo, mid)
        lm = pad_states(lm, hi)
    assert resident(lm[0].shape[0], K, B, C) == (where == "resident")
    refs = make_refs(rng, S, K, 0, 10)
    finals = []
    for sizes in (lambda s, c: 7, lambda s, c: (1, 20, 3)[(s + c) % 3]):
        h = Harness(S, K, T, 0, B, C, N, lm=lm)
        for rows in split(y, lens, sizes):
            h.step(rows)
            h.check(2)
            h.check(1)
        h.check([2, 1, 2], refs=refs)
        finals.append(h.bs.emit([2] * S, nbest=N, refs=refs))
    same(finals[0], finals[1])
    tw = R.BeamStreamTwin(S, K, T, 0, B, C, lm=lm)
    tw.step(y, lens)
    check_twin(finals[0], tw.emit([2] * S, N))
    check_twin(h.bs.emit([1] * S, nbest=N), tw.emit([1] * S, N))


# ---------------------------------------------------------------------------------------------------------------------------------
# dead utterances, class weights, rows that must not be read, a column window
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dead_at", [10, 14, 19])
def test_a_dead_frame_first_in_the_middle_and_last_in_a_chunk(dead_at):
    """chunks of 10: frame 10 opens a chunk, 14 lies inside one, 19 closes one.  From there on the list is the first entry, score -inf"""
    rng = np.random.RandomState(4124 + dead_at)
    S, T, K, B, C, N = 2, 30, 9, 8, 5, 4
    y = softmax_rows(rng, T, S, K)
    y[dead_at, 0] = 0.0
    w = (0.5 + rng.rand(K)).astype(np.float32)
    h = Harness(S, K, T, 0, B, C, N, w=w, window=(3, 40))
    tw = R.BeamStreamTwin(S, K, T, 0, B, C, w=w)
    for rows in split(y, [T, T], lambda s, c: 10):
        h.step(rows)
        res = h.check(1)
        tw.step(np.stack(rows, 1), [10, 10])
        check_twin(res, tw.emit([1, 1], N))
    assert res.nbest_count.cpu().numpy().tolist() == [1, N] and float(res.score[0, 0]) == -np.inf


# ---------------------------------------------------------------------------------------------------------------------------------
# overflow
# ---------------------------------------------------------------------------------------------------------------------------------
def test_max_frames_is_served_and_one_frame_more_is_rejected_with_the_state_intact():
    rng = np.random.RandomState(4125)
    S, K, B, C, N, F = 2, 9, 8, 5, 4, 25
    y = softmax_rows(rng, F + 1, S, K)
    h = Harness(S, K, F, 0, B, C, N)
    h.step([y[:20, 0], y[:12, 1]]); h.check(1)
    h.step([y[20:25, 0], y[12:18, 1]]); before = h.check(1)         # stream 0: max_frames exactly reached
    h.step([y[25:26, 0], y[18:20, 1]], count=False)                 # stream 0 rejected, stream 1 goes on
    h.hist[1] = y[:20, 1]
    after = h.bs.emit([1, 1], nbest=N)
    assert after.frames.cpu().numpy().tolist() == [-1 - 25, 20]
    same(after, before, [0])
    same(after, h.whole(), [0, 1])
    h.step([y[:6, 0], y[20:26, 1]], start=[1, 0], count=False)      # a start clears the flag; stream 1: 20 + 6 > 25, rejected
    h.hist[0] = y[:6, 0]
    again = h.bs.emit([1, 1], nbest=N)
    assert again.frames.cpu().numpy().tolist() == [6, -1 - 20]
    same(again, h.whole(), [0, 1])


# ---------------------------------------------------------------------------------------------------------------------------------
# references: edit distances and the six totals over the finalised streams
# ---------------------------------------------------------------------------------------------------------------------------------
def test_errors_and_totals_cover_the_streams_emitted_with_mode_2():
    import torch
    rng = np.random.RandomState(4126)
    S, T, K, B, C, N = 4, 40, 12, 16, 8, 5
    lens = [40, 31, 8, 40]
    y = softmax_rows(rng, T, S, K)
    refs = make_refs(rng, S, K, 0, 12)
    refs[3] = [1, K, 2]                                             # a label outside [0, K): listed, not counted
    h = Harness(S, K, T, 0, B, C, N)
    tot_s = torch.zeros(6, dtype=torch.float64, device="cuda")
    tot_w = torch.zeros(6, dtype=torch.float64, device="cuda")
    ended = [False] * S
    for rows in split(y, lens, lambda s, c: 8):
        h.step(rows)
        mode = [2 if len(h.hist[s]) == lens[s] and not ended[s] else (1 if s == 0 else 0) for s in range(S)]
        if 2 not in mode:
            continue
        res = h.bs.emit(mode, nbest=N, refs=refs, totals=tot_s)
        fin = [s for s in range(S) if mode[s] == 2]
        # the whole-utterance call on the finalised streams alone (the others idle): the same errors, the same additions
        keep = list(h.hist)
        h.hist = [keep[s] if s in fin else keep[s][:0] for s in range(S)]
        want = h.whole(refs=refs, totals=tot_w)
        h.hist = keep
        same(res, want, fin)
        err = res.errors.cpu().numpy()
        for s in range(S):
            if mode[s] != 2:
                assert err[s].tolist() == [-1] * N
            else:
                ended[s] = True
    torch.cuda.synchronize()
    assert all(ended) and tot_s.cpu().numpy().tolist() == tot_w.cpu().numpy().tolist() and tot_s[3].item() == 3


# ---------------------------------------------------------------------------------------------------------------------------------
# determinism; the stream an utterance sits in does not matter
# ---------------------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits_and_streams_can_be_permuted():
    rng = np.random.RandomState(4127)
    S, T, K, B, C, N = 4, 50, 12, 16, 8, 5
    lens = [50, 33, 7, 41]
    y = softmax_rows(rng, T, S, K)
    perm = [2, 0, 3, 1]

    def go(order):
        h = Harness(S, K, T, 0, B, C, N)
        out = []
        for rows in split(y[:, order], [lens[i] for i in order], lambda s, c: 9):
            h.step(rows)
            out.append(h.bs.emit([1] * S, nbest=N))
        return out
    a, b, c = go(list(range(S))), go(list(range(S))), go(perm)
    for ra, rb, rc in zip(a, b, c):
        for t in ("hyp_len", "nbest_count", "frames", "stable_len"):
            assert getattr(ra, t).cpu().numpy().tolist() == getattr(rb, t).cpu().numpy().tolist()
        same(ra, rb)
        cnt, cc = ra.nbest_count.cpu().numpy(), rc.nbest_count.cpu().numpy()
        ha, hc, na, nc = ra.hyp.cpu().numpy(), rc.hyp.cpu().numpy(), ra.hyp_len.cpu().numpy(), rc.hyp_len.cpu().numpy()
        sa, sc = ra.score.cpu().numpy().view(np.int32), rc.score.cpu().numpy().view(np.int32)
        for j, i in enumerate(perm):                                # stream j of the permuted run carries utterance i
            assert cnt[i] == cc[j] and ra.stable_len[i].item() == rc.stable_len[j].item()
            for q in range(cnt[i]):
                assert ha[i, q, :na[i, q]].tolist() == hc[j, q, :nc[j, q]].tolist() and sa[i, q] == sc[j, q]


# ---------------------------------------------------------------------------------------------------------------------------------
# the stable prefix on the device
# ---------------------------------------------------------------------------------------------------------------------------------
def test_stable_len_is_exact_when_a_prefix_left_the_beam_and_came_back():
    y, lm, B, C = returning_prefix_case()
    h = Harness(1, 3, 3, 0, B, C, B, lm=lm)
    h.step([y[:2, 0]])
    h.step([y[2:, 0]])
    res = h.check(1)
    assert h.k.nbest_to_lists(res)[0][0][0] == [1, 2, 1] and h.k.nbest_to_lists(res)[0][1][0] == [1]
    assert res.stable_len.cpu().numpy().tolist() == [1]


def test_stable_len_equals_the_twins_after_every_chunk():
    rng = np.random.RandomState(4128)
    S, T, K, B, C, N = 3, 48, 7, 8, 4, 8
    y = softmax_rows(rng, T, S, K, scale=3.0)
    h = Harness(S, K, T, 0, B, C, N)
    tw = R.BeamStreamTwin(S, K, T, 0, B, C)
    seen = set()
    for rows in split(y, [T] * S, lambda s, c: 4):
        h.step(rows)
        tw.step(np.stack(rows, 1), [4] * S)
        res = h.bs.emit([1] * S, nbest=N)
        e = tw.emit([1] * S, N)
        check_twin(res, e)
        seen.update(e["stable_len"])
    assert len(seen) > 3                                            # it moves


# ---------------------------------------------------------------------------------------------------------------------------------
# refused arguments launch nothing
# ---------------------------------------------------------------------------------------------------------------------------------
def test_limits_and_null_arguments_return_the_documented_status():
    import ctypes
    import torch
    import kaldi_lstm_amd as k
    lib = k.load_library()
    S, K, B, C, N, F, T = 2, 8, 4, 4, 2, 16, 4
    bs = k.CtcBeamStream(S, K, F, beam=B, cands=C)
    y = torch.from_numpy(softmax_rows(np.random.RandomState(1), T, S, K).reshape(T * S, K)).cuda()
    bs.step(y, [4, 4])
    good = bs.emit([1, 1], nbest=N)
    torch.cuda.synchronize()
    state0 = bs.state.clone()
    lens = torch.tensor([4, 4], dtype=torch.int32, device="cuda")
    ws = torch.empty(k.ctc_beam_stream_workspace_bytes(T, S, C, N), dtype=torch.uint8, device="cuda")
    sz, nbytes = ctypes.c_size_t, ws.numel()

    def step(y=y, T=T, S=S, K=K, lens=lens, B=B, C=C, state=bs.state, nstate=None, F=F, ws=ws, nws=None):
        return lib.klstm_ctc_beam_stream_step(y.data_ptr() if y is not None else None, T, S, K, K, lens.data_ptr() if lens is not None else None,
                                              None, 0, None, B, C, 0, None, None, state.data_ptr() if state is not None else None,
                                              sz(bs.state_bytes if nstate is None else nstate), F, ws.data_ptr() if ws is not None else None,
                                              sz(nbytes if nws is None else nws), None)
    for kw, status in ((dict(y=None), 1), (dict(lens=None), 1), (dict(state=None), 1), (dict(ws=None), 1), (dict(nstate=bs.state_bytes - 1), 1),
                       (dict(nws=nbytes - 1), 1), (dict(S=33), 2), (dict(T=40000), 2), (dict(B=65), 2), (dict(C=8), 2), (dict(F=0), 2)):
        assert step(**kw) == status, kw
    with pytest.raises(k.KlstmError) as ei:
        bs.step(torch.zeros(40000 * S, K, device="cuda"), [1, 1])   # T * S <= 65535 per call
    assert ei.value.status == 2
    out = [torch.full((S * N * F,), -7, dtype=torch.int32, device="cuda"), torch.full((S * N,), -7, dtype=torch.int32, device="cuda"),
           torch.full((S,), -7, dtype=torch.int32, device="cuda")]
    mode = torch.tensor([1, 1], dtype=torch.int32, device="cuda")

    def emit(mode=mode, N=N, stride=F, state=bs.state, hyp=out[0], nws=None):
        return lib.klstm_ctc_beam_stream_emit(S, K, 0, B, N, mode.data_ptr() if mode is not None else None, 0, None,
                                              state.data_ptr() if state is not None else None, sz(bs.state_bytes), F,
                                              hyp.data_ptr() if hyp is not None else None, stride, out[1].data_ptr(), out[2].data_ptr(), None, None,
                                              None, None, None, None, None, ws.data_ptr(), sz(ws.numel() if nws is None else nws), None)
    for kw, status in ((dict(mode=None), 1), (dict(state=None), 1), (dict(hyp=None), 1), (dict(nws=100), 1), (dict(N=B + 1), 2), (dict(stride=F - 1), 2)):
        assert emit(**kw) == status, kw
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in out), "a refused emit wrote an output"
    assert torch.equal(bs.state, state0), "a refused step wrote the state"
    assert emit() == 0
    same(bs.emit([1, 1], nbest=N), good)


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end through the C++ classes (CtcStreamDecoder, BatchScorer::ForEachChunk, DecodeCtcStreaming; tests/cpp/ctc_beam_stream_test)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_cpp_streaming_decode_equals_the_whole_utterance_decoders():
    """The pattern task of the sibling drivers, trained, then streamed at chunk 7 and chunk 20.  The streaming lists equal, bit for bit,
    a CtcBeamDecoder on the posteriors BatchScorer::ForEachChunk handed out, and the DecodeCtcStats agree; against
    DecodeCtcWholeUtterances, whose forward pass runs other kernels, and between the two chunk sizes, whose forward passes run other
    launch plans (the posteriors differ in their last bits), the hypotheses, the edit distances and the statistics agree."""
    from tests.test_ctc_beam_stream import run_driver
    r = run_driver("stream", 7, 20)
    kv = dict(f.split("=") for f in r.stdout.split() if "=" in f)
    print("ctc_beam_stream_test stream 7 20:", r.stdout.strip(), flush=True)
    assert int(kv["captured_same"]) == 1 and int(kv["stats_same"]) == 1 and int(kv["chunkings_same"]) == 1
    assert int(kv["whole_same"]) == 1
    assert int(kv["skipped"]) == 1 and int(kv["scored"]) == 12 and float(kv["ter_whole"]) == 0.0
