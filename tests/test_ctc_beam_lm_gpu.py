"""CTC prefix beam search with a label language model on the GPU (klstm_ctc_beam_decode_lm; kaldi-lstm_amd/csrc/klstm_ctc_beam.hip
k_ctc_beam<1>, <2>) against its numpy twin (tests/ctc_beam_lm_ref.py).  Every integer -- hypotheses, lengths, list sizes, edit
distances, all six totals -- must EQUAL the twin; the probabilities behind a score are bit-identical by construction, so the score may
differ by the device's double log and one rounding only: 2 float32 ulps.  The two places the tables can be read from (global memory,
LDS) must give the same bits."""
import numpy as np
import pytest

from tests import ctc_beam_lm_ref as L
from tests import ctc_decode_ref as D
from tests.test_ctc_beam import grid_case, softmax_rows
from tests.test_ctc_beam_gpu import check, make_refs, ragged_lens, score_bits, to_dev
from tests.test_ctc_beam_lm import bigram_next, forbidden_case, grid_bigram, has_transition, random_trigram, trivial_lm

pytestmark = pytest.mark.gpu


def run_lm(y, lens, blank, B, C, N, lm, w=None, refs=None):
    import torch
    import kaldi_lstm_amd as k
    wd = torch.from_numpy(np.asarray(w, np.float32)).cuda() if w is not None else None
    tot = torch.zeros(6, dtype=torch.float64, device="cuda") if refs is not None else None
    dlm = k.CtcLabelLm(*lm) if lm is not None else None
    res = k.ctc_beam_decode(to_dev(y), lens, blank=blank, beam=B, cands=C, nbest=N, class_weight=wd, refs=refs, totals=tot, lm=dlm)
    torch.cuda.synchronize()
    return res, (tot.cpu().numpy().tolist() if tot is not None else None)


def run_and_check_lm(y, lens, blank, B, C, N, lm, w=None, refs=None, stats=None):
    res, tot = run_lm(y, lens, blank, B, C, N, lm, w, refs)
    tw = L.beam_twin_lm(y, lens, blank, B, C, N, lm, w=w, refs=refs, stats=stats)
    check(res, tot, tw, N)
    return res, tw


def same_bits(ra, rb):
    """two results hold the same lists: counts, lengths, tokens, score bits, errors"""
    cnt = ra.nbest_count.cpu().numpy()
    assert cnt.tolist() == rb.nbest_count.cpu().numpy().tolist()
    ha, hb, na, nb = ra.hyp.cpu().numpy(), rb.hyp.cpu().numpy(), ra.hyp_len.cpu().numpy(), rb.hyp_len.cpu().numpy()
    for s in range(len(cnt)):
        for q in range(cnt[s]):
            assert na[s, q] == nb[s, q] and ha[s, q, :na[s, q]].tolist() == hb[s, q, :na[s, q]].tolist(), (s, q)
            assert score_bits(ra)[s, q] == score_bits(rb)[s, q], (s, q)
    if ra.errors is not None:
        assert ra.errors.cpu().numpy().tolist() == rb.errors.cpu().numpy().tolist()


def resident(Q, K, B, C):
    import kaldi_lstm_amd as k
    return bool(k.load_library().klstm_ctc_beam_lm_resident(Q, K, B, C))


def random_bigram(rng, K, zero=0.2, final=True):
    wt = np.exp(rng.randn(K + 1, K)).astype(np.float32)
    wt[rng.rand(K + 1, K) < zero] = 0.0
    return bigram_next(K), wt, ((0.05 + rng.rand(K + 1)).astype(np.float32) if final else None)


def pad_states(lm, Q):
    """the same automaton with unreachable states behind it"""
    nxt, wt, fin = lm
    q0, K = nxt.shape
    rng = np.random.RandomState(Q)
    nx = np.concatenate([nxt, rng.randint(0, Q, (Q - q0, K)).astype(np.int32)])
    w2 = np.concatenate([wt, rng.rand(Q - q0, K).astype(np.float32)])
    f2 = np.concatenate([fin, rng.rand(Q - q0).astype(np.float32)]) if fin is not None else None
    return nx, w2, f2


# ---------------------------------------------------------------------------------------------------------------------------------
# the trivial LM: the bits of klstm_ctc_beam_decode
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,T,K,B,C,N", [(4, 120, 12, 16, 8, 5), (1, 40, 48, 64, 32, 64)])
def test_trivial_lm_gives_the_bits_of_the_call_without_one(S, T, K, B, C, N):
    rng = np.random.RandomState(S * 1000 + T)
    lens = ragged_lens(rng, S, T)
    y = softmax_rows(rng, T, S, K)
    refs = make_refs(rng, S, K, 0, 12)
    ra, ta = run_lm(y, lens, 0, B, C, N, None, refs=refs)
    rb, tb = run_lm(y, lens, 0, B, C, N, trivial_lm(K), refs=refs)
    same_bits(ra, rb)
    assert ta == tb


# ---------------------------------------------------------------------------------------------------------------------------------
# bigram and trigram tables on ragged streams: the 64-, 128- and 256-thread plans, several keys a thread, tables in LDS and in global
# memory; with and without final weights and class weights, the blank first, in the middle and last
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bigram", "trigram"])
@pytest.mark.parametrize("S,T,K,B,C,N", [(1, 50, 29, 8, 6, 8), (8, 60, 12, 8, 5, 3), (32, 24, 7, 4, 3, 2), (1, 40, 48, 64, 32, 64)])
def test_ngram_tables_on_ragged_streams(kind, S, T, K, B, C, N):
    rng = np.random.RandomState(S * 1000 + T + len(kind))
    lens = ragged_lens(rng, S, T)
    y = softmax_rows(rng, T, S, K)
    for s in range(S):
        y[lens[s]:, s] = np.nan                                  # padding rows and idle streams are not read
    combos = [("first", True, False), ("middle", False, True), ("last", True, True), ("first", False, False)]
    for where, final, weights in combos:
        blank = dict(first=0, middle=K // 2, last=K - 1)[where]
        lm = random_bigram(rng, K, final=final) if kind == "bigram" else random_trigram(rng, K, final=final)
        w = (0.5 + rng.rand(K)).astype(np.float32) if weights else None
        run_and_check_lm(y, lens, blank, B, C, N, lm, w=w, refs=make_refs(rng, S, K, blank, 12))


# lists of 16, 108, 144, 200 and 768 entries: 64, 128 and 256 threads, one key and several keys a thread
@pytest.mark.parametrize("K,B,C", [(29, 16, 8), (12, 4, 3), (12, 12, 8), (12, 40, 4), (12, 64, 11)])
def test_both_sides_of_the_resident_threshold(K, B, C):
    """the same automaton, padded with unreachable states until the tables no longer go to LDS: the same bits, and the twin's on
    both sides"""
    rng = np.random.RandomState(31)
    S, T, N = 3, 40, min(B, 6)
    lens = [40, 23, 1]
    y = softmax_rows(rng, T, S, K)
    refs = make_refs(rng, S, K, 0, 10)
    lm = random_bigram(rng, K)
    lo, hi = K + 1, (1 << 24) // K
    assert resident(lo, K, B, C) and not resident(hi, K, B, C)
    while hi - lo > 1:                                            # the last resident state count
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if resident(mid, K, B, C) else (lo, mid)
    small, big = pad_states(lm, lo), pad_states(lm, hi)
    assert small[0].shape[0] == lo and big[0].shape[0] == hi
    ra, tw = run_and_check_lm(y, lens, 0, B, C, N, lm, refs=refs)
    rb, _ = run_lm(y, lens, 0, B, C, N, small, refs=refs)
    same_bits(ra, rb)
    rb, _ = run_and_check_lm(y, lens, 0, B, C, N, big, refs=refs)
    same_bits(ra, rb)


def test_resident_tables_between_32_and_64_kb():
    """a character bigram at K = 64 (33280 bytes of tables) and the same automaton padded to 59904 bytes: the tables go to LDS, and
    with the kernel's own 31 KB the launch needs more than 64 KB of LDS while its dynamic part alone stays below that"""
    rng = np.random.RandomState(33)
    S, T, K, B, C, N = 2, 30, 64, 8, 6, 4
    lens = [30, 19]
    y = softmax_rows(rng, T, S, K)
    refs = make_refs(rng, S, K, 0, 10)
    lm = random_bigram(rng, K)
    padded = pad_states(lm, 117)
    for tab in (lm, padded):
        nbytes = tab[0].size * 8
        assert 32 * 1024 < nbytes <= 64 * 1024 and resident(tab[0].shape[0], K, B, C)
    ra, _ = run_and_check_lm(y, lens, 0, B, C, N, lm, refs=refs)
    rb, _ = run_lm(y, lens, 0, B, C, N, padded, refs=refs)
    same_bits(ra, rb)


# ---------------------------------------------------------------------------------------------------------------------------------
# merges: an extension that equals a prefix of the beam carries its LM factor into that entry's sum
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 5, 13, 20, 8])
def test_merged_extensions_carry_the_lm_factor(seed):
    y, K, T, B, C = grid_case(seed)
    stats = {}
    res, tw = run_and_check_lm(y, [T], 0, 16, C, 16, grid_bigram(seed, K, final=seed % 4 == 1), stats=stats)
    assert stats["merges"] > 0                                    # the case covers what it is named for
    hy = [tuple(h) for h in tw["hyp"][0]]
    assert len(set(hy)) == len(hy)


def test_peaked_posteriors_with_repeats():
    rng = np.random.RandomState(41)
    S, T, K = 4, 48, 9
    lens = [48, 30, 0, 17]
    refs = [[1, 1, 2, 3, 3, 3, 1], [4, 4, 5], [], [6, 7, 7]]
    y = D.peaked_case(41, T, K, 0, refs, lens, [(1, 0, 1, 1), (0, 1, 0, 1), (0, 0, 0, 0), (1, 1, 1, 0)])
    stats = {}
    run_and_check_lm(y, lens, 0, 8, 5, 4, random_bigram(rng, K, zero=0.1), refs=refs, stats=stats)
    assert stats["merges"] > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# forbidden extensions: weight 0 and next outside [0, Q)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 3, 6, 9])
def test_zero_weights_and_out_of_range_next(seed):
    y, K, T, B, C, nxt, lm, forb = forbidden_case(seed)
    res, tw = run_and_check_lm(y, [T], 0, B, C, B, lm)
    n = int(res.nbest_count[0])
    h, hl = res.hyp.cpu().numpy()[0], res.hyp_len.cpu().numpy()[0]
    for q, c in zip(*np.nonzero(forb[:, 1:])):
        assert not any(has_transition(nxt, h[i, :hl[i]].tolist(), q, c + 1) for i in range(n)), (q, c + 1)


def test_a_fully_forbidden_utterance_is_dead():
    rng = np.random.RandomState(43)
    S, T, K = 3, 12, 6
    y = softmax_rows(rng, T, S, K)
    y[4, :, 0] = 0.0                                              # a frame without the blank: a label must be emitted
    nxt = bigram_next(K)
    wt = np.ones((K + 1, K), np.float32)
    for lm in ((nxt, np.zeros_like(wt), None), (np.full_like(nxt, -1), wt, None), (np.full_like(nxt, K + 1), wt, np.ones(K + 1, np.float32)),
               (nxt, wt, np.zeros(K + 1, np.float32))):
        res, tw = run_and_check_lm(y, [T, 3, T], 0, 4, 3, 4, lm, refs=[[1], [2, 3], []])
        assert tw["nbest_count"][0] == 1 and tw["score"][0] == [-np.inf] and res.score.cpu().numpy()[0, 0] == -np.inf


# ---------------------------------------------------------------------------------------------------------------------------------
# edge parameters
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,B,C,N", [(9, 1, 4, 1), (9, 6, 1, 3), (9, 5, 8, 5), (9, 7, 3, 7), (2, 4, 1, 4), (2, 1, 1, 1)])
def test_edge_parameters(K, B, C, N):
    """B = 1, C = 1, C = K - 1, N = B, K = 2; a bigram, and Q = 1 (a unigram with a final weight)"""
    rng = np.random.RandomState(K * 100 + B * 10 + C)
    S, T = 3, 30
    lens = [30, 17, 1]
    y = softmax_rows(rng, T, S, K, scale=1.0)
    refs = make_refs(rng, S, K, K - 1, 8)
    run_and_check_lm(y, lens, K - 1, B, C, N, random_bigram(rng, K, zero=0.1), refs=refs)
    unigram = (np.zeros((1, K), np.int32), np.exp(rng.randn(1, K)).astype(np.float32), np.array([0.5], np.float32))
    run_and_check_lm(y, lens, K - 1, B, C, N, unigram, refs=refs)


# ---------------------------------------------------------------------------------------------------------------------------------
# determinism
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bigram", "trigram"])
def test_bit_identical_across_runs_and_streams(kind):
    """the same utterance in stream 0 of S = 1 and in stream 5 of S = 8, among different neighbours; and twice"""
    rng = np.random.RandomState(45)
    T, K, B, C, N = 40, 29, 16, 8, 6
    lm = random_bigram(rng, K) if kind == "bigram" else random_trigram(rng, K)
    y8 = softmax_rows(rng, T, 8, K)
    lens8 = [40, 0, 1, 33, 40, 27, 12, 40]
    ra, _ = run_lm(y8, lens8, 0, B, C, N, lm)
    rb, _ = run_lm(y8, lens8, 0, B, C, N, lm)
    same_bits(ra, rb)
    y1 = np.full((T, 1, K), np.nan, np.float32)
    y1[:27, 0] = y8[:27, 5]
    rc, _ = run_lm(y1, [27], 0, B, C, N, lm)
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
    import ctypes
    import torch
    import kaldi_lstm_amd as k
    lib = k.load_library()
    T, S, K, B, C, N = 4, 2, 8, 4, 4, 2
    y = torch.full((T * S, K), 0.125, device="cuda")
    lens = torch.tensor([4, 3], dtype=torch.int32, device="cuda")
    nxt = torch.zeros(2, K, dtype=torch.int32, device="cuda")
    wt = torch.ones(2, K, device="cuda")
    nbytes = k.ctc_beam_workspace_bytes(T, S, B, C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    hyp = torch.full((S, N, T), -7, dtype=torch.int32, device="cuda")
    hlen = torch.full((S, N), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((S,), -7, dtype=torch.int32, device="cuda")
    score = torch.full((S, N), -7.0, device="cuda")

    def call(Q, nx, w):
        st = lib.klstm_ctc_beam_decode_lm(y.data_ptr(), T, S, K, K, lens.data_ptr(), 0, None, B, C, N, Q, nx, w, None, hyp.data_ptr(),
                                          hlen.data_ptr(), cnt.data_ptr(), score.data_ptr(), None, None, None, None, ws.data_ptr(),
                                          ctypes.c_size_t(nbytes), None)
        torch.cuda.synchronize()
        return st
    assert call((1 << 24) // K + 1, nxt.data_ptr(), wt.data_ptr()) == 2          # KLSTM_ERR_SHAPE
    assert call(2, nxt.data_ptr(), None) == 1                                    # KLSTM_ERR_ARG
    assert call(2, None, wt.data_ptr()) == 1 and call(0, nxt.data_ptr(), wt.data_ptr()) == 2
    assert bool((hyp == -7).all()) and bool((hlen == -7).all()) and bool((cnt == -7).all()) and bool((score == -7).all())
    assert call(2, nxt.data_ptr(), wt.data_ptr()) == 0                           # and the call itself is fine
    assert cnt.tolist() == [N, N]


# ---------------------------------------------------------------------------------------------------------------------------------
# the C++ classes (include/klstm_nnet.hpp CtcLabelLm, CtcBeamDecoder::SetLanguageModel, DecodeCtcOptions::lm; tests/cpp/ctc_beam_lm_test)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_cpp_decoder_and_options_equal_the_python_path(tmp_path):
    from tests.test_ctc_beam_lm import run_driver
    rng = np.random.RandomState(47)
    T, S, K, B, C, N = 30, 4, 9, 8, 5, 4
    lens = [30, 0, 11, 24]
    y = softmax_rows(rng, T, S, K)
    lm = random_bigram(rng, K)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as fh:
        np.array([T, S, K, B, C, N, K + 1, 1, 0] + lens, np.int32).tofile(fh)
        y.tofile(fh)
        lm[0].astype(np.int32).tofile(fh); lm[1].tofile(fh); lm[2].tofile(fh)
    r = run_driver("decode", src, dst)
    assert "best_ok=1" in r.stdout
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
    with_lm, _ = run_and_check_lm(y, lens, 0, B, C, N, lm)
    without, _ = run_lm(y, lens, 0, B, C, N, None)
    assert passes[0] == as_lists(with_lm) and passes[1] == as_lists(with_lm)
    assert passes[2] == as_lists(without) and passes[3] == as_lists(without)
    assert passes[0] != passes[2]                                 # the LM does change these lists
