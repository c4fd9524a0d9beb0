"""The CTC beam search with a sparse back-off language model on the GPU (klstm_ctc_slm_build, klstm_ctc_beam_decode_slm,
klstm_ctc_beam_stream_step_slm; kaldi-lstm_amd/csrc/klstm_ctc_beam.hip k_ctc_beam<3>, k_ctc_beam_stream<3>, k_slm_*).  Two bars:
  against the dense call on the expansion of the model (ctc_beam_decode(lm=CtcLabelLm(*sparse_lm_to_dense(m)))): EQUALITY of every
  output field, score bits included -- a lookup is defined as the value the expansion holds, so there is no tolerance;
  against the twin (tests/ctc_beam_slm_ref.py: beam_twin_lm on the expansion, or on lazy tables for a model too large to expand):
  every integer equal, scores within 2 float32 ulps (the device's double log and one rounding), the bar of the dense LM tests."""
import ctypes

import numpy as np
import pytest

from tests import ctc_beam_slm_ref as R
from tests import margins
from tests.test_ctc_beam import softmax_rows
from tests.test_ctc_beam_gpu import check, make_refs, ragged_lens, score_bits, to_dev
from tests.test_ctc_beam_lm_gpu import same_bits
from tests.test_ctc_beam_stream_gpu import same, split

pytestmark = pytest.mark.gpu


def decode(y, lens, blank, B, C, N, dlm, w=None, refs=None):
    """dlm: a CtcSparseLabelLm, a CtcLabelLm or None"""
    import torch
    import kaldi_lstm_amd as k
    wd = torch.from_numpy(np.asarray(w, np.float32)).cuda() if w is not None else None
    tot = torch.zeros(6, dtype=torch.float64, device="cuda") if refs is not None else None
    res = k.ctc_beam_decode(to_dev(y), lens, blank=blank, beam=B, cands=C, nbest=N, class_weight=wd, refs=refs, totals=tot, lm=dlm)
    torch.cuda.synchronize()
    return res, (tot.cpu().numpy().tolist() if tot is not None else None)


def sparse_on_device(model, blank, final="model"):
    import kaldi_lstm_amd as k
    return k.CtcSparseLabelLm(model, blank, final=final)


def dense_on_device(model, final="model"):
    import kaldi_lstm_amd as k
    nxt, wt, _ = k.sparse_lm_to_dense(model)
    return k.CtcLabelLm(nxt, wt, R.final_of(model, final))


def check_twin(res, tot, tw, N):
    margins.bound(check(res, tot, tw, N), 2, "score ulps against the twin")


def clean(dlm):
    assert dlm.status_list()[:6] == [0] * 6 and dlm.status_list()[7] == 0
    return dlm


# ---------------------------------------------------------------------------------------------------------------------------------
# sparse against dense, bit for bit, and against the twin: a model without any back-off, a bigram, an order-5 model; ragged streams;
# the 64-, 128- and 256-thread plans; with and without final and class weights; the blank first, in the middle and last
# ---------------------------------------------------------------------------------------------------------------------------------
def model_of(kind, seed, K, blank, final):
    if kind == "explicit":
        return R.explicit_model(np.random.RandomState(seed), K, blank, 9, final=final)
    m = R.counted_model(seed, K, blank, 2 if kind == "bigram" else 5)
    return m if final else R.without_final(m)


@pytest.mark.parametrize("kind", ["explicit", "bigram", "order5"])
@pytest.mark.parametrize("S,T,K,B,C,N", [(1, 50, 29, 8, 6, 8), (8, 60, 12, 8, 5, 3), (32, 24, 7, 4, 3, 2), (1, 40, 48, 64, 32, 64)])
def test_sparse_equals_dense_on_the_expansion_and_the_twin(kind, S, T, K, B, C, N):
    rng = np.random.RandomState(S * 1000 + T + len(kind))
    lens = ragged_lens(rng, S, T)
    y = softmax_rows(rng, T, S, K)
    for s in range(S):
        y[lens[s]:, s] = np.nan                                  # padding rows and idle streams are not read
    combos = [("first", True, False), ("middle", False, True), ("last", True, True), ("first", False, False)]
    for i, (where, final, weights) in enumerate(combos):
        blank = dict(first=0, middle=K // 2, last=K - 1)[where]
        model = model_of(kind, S + i, K, blank, final)
        w = (0.5 + rng.rand(K)).astype(np.float32) if weights else None
        refs = make_refs(rng, S, K, blank, 12)
        dlm = clean(sparse_on_device(model, blank))
        rs, ts = decode(y, lens, blank, B, C, N, dlm, w=w, refs=refs)
        rd, td = decode(y, lens, blank, B, C, N, dense_on_device(model), w=w, refs=refs)
        same_bits(rs, rd)
        assert ts == td
        if i == (len(kind) + S) % 4:                              # one combination a case goes through the twin as well
            tw, _ = R.beam_twin_slm(y, lens, blank, B, C, N, model, w=w, refs=refs)
            check_twin(rs, ts, tw, N)
        if kind == "explicit":
            assert np.all(np.asarray(model.backoff) == -1)
        else:
            assert dlm.status_list()[6] >= 1                      # the empty history has every label: a direct row


# ---------------------------------------------------------------------------------------------------------------------------------
# back-off coverage: the seeds tests/test_ctc_beam_slm.py holds to the same condition on the CPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", R.COVERAGE_SEEDS)
def test_backoffs_of_every_depth_are_taken_and_the_lm_changes_the_one_best(seed):
    sh = R.COVERAGE_SHAPE
    y, lens, model = R.coverage_case(seed)
    tw, tabs = R.beam_twin_slm(y, lens, sh["blank"], sh["B"], sh["C"], sh["N"], model, lazy=True)
    missing, changed, weakest = R.coverage_findings(y, lens, model, tw, tabs)
    assert weakest >= R.STRONG and missing == [] and changed != [], (dict(tabs.depth), changed)
    res, _ = decode(y, lens, sh["blank"], sh["B"], sh["C"], sh["N"], clean(sparse_on_device(model, sh["blank"])))
    check_twin(res, None, tw, sh["N"])
    plain, _ = decode(y, lens, sh["blank"], sh["B"], sh["C"], sh["N"], None)
    s = changed[0]
    n = int(res.hyp_len[s, 0])
    assert n != int(plain.hyp_len[s, 0]) or res.hyp[s, 0, :n].tolist() != plain.hyp[s, 0, :n].tolist()


# ---------------------------------------------------------------------------------------------------------------------------------
# a model the dense form cannot hold in a test's budget: K = 256, order 4, some 10^4 states; the twin answers through lazy tables
# ---------------------------------------------------------------------------------------------------------------------------------
def test_a_model_too_large_for_dense_tables():
    import kaldi_lstm_amd as k
    K, blank, S, T, B, C, N = 256, 0, 2, 30, 8, 6, 4
    rng = np.random.RandomState(77)
    model = k.backoff_ngram_label_lm(R.chain_sequences(rng, K, blank, 3000, 8), K, blank, order=4, alpha=0.9, beta=0.5)
    Q = len(model.backoff)
    assert Q >= 10000 and Q * K * 8 > 20 * 2 ** 20                # the dense tables would be tens of MB
    y = softmax_rows(rng, T, S, K, scale=3.0)
    lens = [30, 21]
    refs = make_refs(rng, S, K, blank, 10)
    dlm = clean(sparse_on_device(model, blank))
    res, tot = decode(y, lens, blank, B, C, N, dlm, refs=refs)
    tw, tabs = R.beam_twin_slm(y, lens, blank, B, C, N, model, refs=refs, lazy=True)
    check_twin(res, tot, tw, N)
    assert sum(tabs.depth[d] for d in (1, 2, 3)) > 0 and tabs.depth[0] > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# forbidding: a miss at a state without back-off, zero arc weights, zero back-off weights; a fully forbidden utterance is dead
# ---------------------------------------------------------------------------------------------------------------------------------
def test_misses_and_zero_weights_forbid():
    import kaldi_lstm_amd as k
    rng = np.random.RandomState(51)
    S, T, K, blank, B, C, N = 3, 30, 8, 0, 8, 5, 8
    y = softmax_rows(rng, T, S, K)
    lens = [30, 12, 21]
    m = R.counted_model(4, K, blank, 3)
    holes = m._replace(backoff=np.where(np.arange(len(m.backoff)) % 3 == 2, -1, m.backoff))           # misses there forbid
    zero_arcs = m._replace(arc_weight=np.where(rng.rand(len(m.arc_weight)) < 0.3, 0, m.arc_weight).astype(np.float32))
    zero_bows = m._replace(backoff_weight=np.where(np.arange(len(m.backoff)) % 2 == 0, 0, m.backoff_weight).astype(np.float32))
    for model in (holes, zero_arcs, zero_bows):
        nxt, wt, _ = k.sparse_lm_to_dense(model)
        assert np.any((wt[:, 1:] == 0) | (nxt[:, 1:] < 0))         # the model does forbid something
        res, tot = decode(y, lens, blank, B, C, N, clean(sparse_on_device(model, blank)))
        tw, _ = R.beam_twin_slm(y, lens, blank, B, C, N, model)
        check_twin(res, tot, tw, N)
        h, hl = res.hyp.cpu().numpy(), res.hyp_len.cpu().numpy()
        for s in range(S):
            for i in range(int(res.nbest_count[s])):
                q = 0
                for c in h[s, i, :hl[s, i]]:
                    assert wt[q, c] > 0 and nxt[q, c] >= 0, (s, i)  # no listed hypothesis took a forbidden step
                    q = int(nxt[q, c])


def test_a_fully_forbidden_utterance_is_dead():
    import kaldi_lstm_amd as k
    rng = np.random.RandomState(43)
    S, T, K = 3, 12, 6
    y = softmax_rows(rng, T, S, K)
    y[4, :, 0] = 0.0                                              # a frame without the blank: a label must be emitted
    m = R.counted_model(5, K, 0, 3)
    Q = len(m.backoff)
    empty = k.SparseLm(K, np.asarray([0, 1] + [1] * (Q - 1)), np.asarray([1]), np.asarray([-1]), np.asarray([1.0], np.float32),
                       np.full(Q, -1), np.ones(Q, np.float32), None)                     # one arc, and it leads nowhere
    for model in (m._replace(arc_weight=np.zeros_like(m.arc_weight)), m._replace(arc_next=np.full_like(m.arc_next, Q)),
                  m._replace(final=np.zeros_like(m.final)), empty):
        res, tot = decode(y, [T, 3, T], 0, 4, 3, 4, clean(sparse_on_device(model, 0)), refs=[[1], [2, 3], []])
        tw, _ = R.beam_twin_slm(y, [T, 3, T], 0, 4, 3, 4, model, refs=[[1], [2, 3], []])
        check_twin(res, tot, tw, 4)
        assert tw["nbest_count"][0] == 1 and tw["score"][0] == [-np.inf] and res.score.cpu().numpy()[0, 0] == -np.inf


# ---------------------------------------------------------------------------------------------------------------------------------
# build validation: built, read back and decoded once each; the outputs are the twin's on the model as cut
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.broken_models()))
def test_the_build_drops_and_cuts_what_it_must(name):
    import kaldi_lstm_amd as k
    model, status = R.broken_models()[name]
    K, blank = R.BROKEN_K, R.BROKEN_BLANK
    cut, mirrored = k.sparse_lm_validate(model, blank)
    dlm = sparse_on_device(model, blank)
    got = dlm.status_list()
    assert got[:6] == status and got == mirrored
    rng = np.random.RandomState(len(name))
    S, T, B, C, N = 2, 24, 8, 5, 4
    y = softmax_rows(rng, T, S, K)
    res, tot = decode(y, [24, 15], blank, B, C, N, dlm)
    tw, _ = R.beam_twin_slm(y, [24, 15], blank, B, C, N, cut)
    check_twin(res, tot, tw, N)


# ---------------------------------------------------------------------------------------------------------------------------------
# streaming: any chunking emits the bits of the whole-utterance sparse call
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1, 7, 40])
def test_streaming_emits_the_bits_of_the_whole_utterance_call(chunk):
    import kaldi_lstm_amd as k
    rng = np.random.RandomState(61)
    S, T, K, blank, B, C, N = 4, 40, 12, 5, 8, 5, 4
    lens = ragged_lens(rng, S, T)                                   # 40, idle, 1, random
    y = softmax_rows(rng, T, S, K)
    model = R.counted_model(6, K, blank, 5)
    dlm, bare = clean(sparse_on_device(model, blank)), sparse_on_device(model, blank, final=None)
    refs = make_refs(rng, S, K, blank, 10)
    bs = k.CtcBeamStream(S, K, T, blank=blank, beam=B, cands=C, lm=dlm)
    done = [0] * S
    for rows in split(y, lens, lambda s, c: chunk):
        cl = [len(r) for r in rows]
        part = np.full((max(max(cl), 1), S, K), np.nan, np.float32)
        for s, r in enumerate(rows):
            part[:len(r), s] = r
        bs.step(to_dev(part), cl)
        done = [d + n for d, n in zip(done, cl)]
        if chunk == 1 and max(done) % 13 and max(done) != T:
            continue                                              # frame by frame: every 13th partial result
        for mode, whole_lm in ((2, dlm), (1, bare)):
            res = bs.emit([mode] * S, nbest=N, refs=refs)
            whole = k.ctc_beam_decode(to_dev(y), done, blank=blank, beam=B, cands=C, nbest=N, refs=refs, lm=whole_lm)
            same(res, whole, errors=(mode == 2))
            assert res.frames.cpu().numpy().tolist() == done
    assert done == lens
    dense = k.ctc_beam_decode(to_dev(y), lens, blank=blank, beam=B, cands=C, nbest=N, refs=refs, lm=dense_on_device(model))
    same(bs.emit([2] * S, nbest=N, refs=refs), dense)


# ---------------------------------------------------------------------------------------------------------------------------------
# determinism
# ---------------------------------------------------------------------------------------------------------------------------------
def test_bit_identical_across_runs_builds_and_streams():
    """the same utterance in stream 0 of S = 1 and in stream 5 of S = 8, among different neighbours; twice; and from a second build"""
    rng = np.random.RandomState(45)
    T, K, B, C, N = 40, 29, 16, 8, 6
    model = R.counted_model(7, K, 0, 5)
    dlm = clean(sparse_on_device(model, 0))
    y8 = softmax_rows(rng, T, 8, K)
    lens8 = [40, 0, 1, 33, 40, 27, 12, 40]
    ra, _ = decode(y8, lens8, 0, B, C, N, dlm)
    rb, _ = decode(y8, lens8, 0, B, C, N, dlm)
    same_bits(ra, rb)
    rb, _ = decode(y8, lens8, 0, B, C, N, sparse_on_device(model, 0))
    same_bits(ra, rb)
    y1 = np.full((T, 1, K), np.nan, np.float32)
    y1[:27, 0] = y8[:27, 5]
    rc, _ = decode(y1, [27], 0, B, C, N, dlm)
    n = int(ra.nbest_count[5])
    assert n == int(rc.nbest_count[0]) and n > 1
    for q in range(n):
        m = int(ra.hyp_len[5, q])
        assert m == int(rc.hyp_len[0, q]) and ra.hyp[5, q, :m].tolist() == rc.hyp[0, q, :m].tolist()
        assert score_bits(ra)[5, q] == score_bits(rc)[0, q]


# ---------------------------------------------------------------------------------------------------------------------------------
# refused arguments
# ---------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks_leave_the_outputs_alone():
    import torch
    import kaldi_lstm_amd as k
    lib = k.load_library()
    T, S, K, B, C, N = 4, 2, 8, 4, 4, 2
    y = torch.full((T * S, K), 0.125, device="cuda")
    lens = torch.tensor([4, 3], dtype=torch.int32, device="cuda")
    dlm = sparse_on_device(R.explicit_model(np.random.RandomState(1), K, 0, 3, zero=0.0), 0)
    other = sparse_on_device(R.explicit_model(np.random.RandomState(1), K + 1, 0, 3, zero=0.0), 0)          # built for 9 classes
    nbytes = k.ctc_beam_workspace_bytes(T, S, B, C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    hyp = torch.full((S, N, T), -7, dtype=torch.int32, device="cuda")
    hlen = torch.full((S, N), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((S,), -7, dtype=torch.int32, device="cuda")
    score = torch.full((S, N), -7.0, device="cuda")
    state_bytes = k.ctc_beam_stream_state_bytes(T, S, B)
    state = torch.zeros(state_bytes, dtype=torch.uint8, device="cuda")
    sws_bytes = k.ctc_beam_stream_workspace_bytes(T, S, C, N)
    sws = torch.empty(sws_bytes, dtype=torch.uint8, device="cuda")

    def call(blob, bytes_, Q):
        st = lib.klstm_ctc_beam_decode_slm(y.data_ptr(), T, S, K, K, lens.data_ptr(), 0, None, B, C, N, blob, ctypes.c_size_t(bytes_), Q, None,
                                           hyp.data_ptr(), hlen.data_ptr(), cnt.data_ptr(), score.data_ptr(), None, None, None, None,
                                           ws.data_ptr(), ctypes.c_size_t(nbytes), None)
        torch.cuda.synchronize()
        return st

    def step(blob, bytes_, Q):
        st = lib.klstm_ctc_beam_stream_step_slm(y.data_ptr(), T, S, K, K, lens.data_ptr(), None, 0, None, B, C, blob, ctypes.c_size_t(bytes_), Q,
                                                state.data_ptr(), ctypes.c_size_t(state_bytes), T, sws.data_ptr(), ctypes.c_size_t(sws_bytes),
                                                None)
        torch.cuda.synchronize()
        return st
    ptr, nb, Q = dlm.blob.data_ptr(), dlm.nbytes, dlm.states
    for fn in (call, step):
        assert fn(None, nb, Q) == 1                                # KLSTM_ERR_ARG: a null blob
        assert fn(ptr, nb - 1, Q) == 1 and fn(ptr, 0, Q) == 1      # wrong bytes
        assert fn(other.blob.data_ptr(), other.nbytes, other.states) == 1            # K of the blob is not K of the call
        assert fn(ptr, nb, Q + 1) == 1                             # nor were these the states it was built for
        assert fn(ptr + 16, nb, Q) == 1                            # not an address a build wrote to
        assert fn(ptr, nb, 0) == 2 and fn(ptr, nb, (1 << 24) + 1) == 2               # KLSTM_ERR_SHAPE
    assert bool((hyp == -7).all()) and bool((hlen == -7).all()) and bool((cnt == -7).all()) and bool((score == -7).all())
    assert bool((state == 0).all())
    assert call(ptr, nb, Q) == 0 and step(ptr, nb, Q) == 0         # and the calls themselves are fine
    assert cnt.tolist() == [N, N]
    # the build's own checks: nothing is written to the blob
    blob = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    arr = torch.zeros(64, dtype=torch.int32, device="cuda")

    def build(states=3, arcs=21, K_=K, blank=0, off=arr, out=blob, out_bytes=nb):
        st = lib.klstm_ctc_slm_build(states, arcs, K_, blank, off.data_ptr() if off is not None else None, arr.data_ptr(), arr.data_ptr(),
                                     arr.data_ptr(), arr.data_ptr(), arr.data_ptr(), out.data_ptr() if out is not None else None,
                                     ctypes.c_size_t(out_bytes), None, None)
        torch.cuda.synchronize()
        return st
    assert build(off=None) == 1 and build(out=None) == 1 and build(out_bytes=nb - 1) == 1 and build(blank=K) == 1 and build(blank=-1) == 1
    assert build(states=0) == 1 and build(states=(1 << 24) + 1) == 2 and build(K_=1) == 2
    assert bool((blob == 0).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# the C++ classes (include/klstm_nnet.hpp ReadArpaLabelLm, CtcSparseLabelLm, the SetLanguageModel overloads, DecodeCtcOptions::slm)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_cpp_reader_and_decoders_equal_the_python_path(tmp_path):
    import kaldi_lstm_amd as k
    from tests.test_ctc_beam_slm import ARPA_BLANK, ARPA_K, ARPA_SYMBOLS, arpa_text, run_driver
    rng = np.random.RandomState(47)
    T, S, K, B, C, N, alpha, beta = 30, 4, ARPA_K, 8, 5, 4, 0.9, 0.2
    lens = [30, 0, 11, 24]
    y = softmax_rows(rng, T, S, K)
    arpa, syms, src, dst = (str(tmp_path / n) for n in ("lm.arpa", "syms.txt", "in.bin", "out.bin"))
    with open(arpa, "w") as fh:
        fh.write(arpa_text())
    with open(syms, "w") as fh:
        fh.write("".join("%s %d\n" % kv for kv in ARPA_SYMBOLS.items()))
    with open(src, "wb") as fh:
        np.array([T, S, B, C, N] + lens, np.int32).tofile(fh)
        y.tofile(fh)
    r = run_driver("decode", arpa, syms, K, ARPA_BLANK, alpha, beta, src, dst, 7)
    assert "best_ok=1" in r.stdout and "dropped=0 cut=0" in r.stdout
    raw = np.fromfile(dst, dtype=np.int32)
    p = 0
    passes = []
    for _ in range(4):
        lists = []
        for s in range(S):
            n = int(raw[p]); p += 1
            ls = []
            for _ in range(n):
                m, bits = int(raw[p]), int(raw[p + 1])
                ls.append((raw[p + 2:p + 2 + m].tolist(), bits))
                p += 2 + m
            lists.append(ls)
        passes.append(lists)
    assert p == len(raw)

    def as_lists(res):
        cnt, h, hl, sb = res.nbest_count.tolist(), res.hyp.cpu().numpy(), res.hyp_len.cpu().numpy(), score_bits(res)
        return [[(h[s, q, :hl[s, q]].tolist(), int(sb[s, q])) for q in range(cnt[s])] for s in range(S)]
    model = k.arpa_label_lm(arpa, ARPA_SYMBOLS, K, ARPA_BLANK, alpha=alpha, beta=beta)
    with_lm, tot = decode(y, lens, ARPA_BLANK, B, C, N, clean(sparse_on_device(model, ARPA_BLANK)))
    tw, _ = R.beam_twin_slm(y, lens, ARPA_BLANK, B, C, N, model)
    check_twin(with_lm, tot, tw, N)
    without, _ = decode(y, lens, ARPA_BLANK, B, C, N, None)
    assert passes[0] == as_lists(with_lm) and passes[1] == as_lists(with_lm) and passes[2] == as_lists(with_lm)
    assert passes[3] == as_lists(without)
    assert passes[0] != passes[3]                                 # the LM does change these lists
