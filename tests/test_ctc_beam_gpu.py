"""CTC prefix beam search on the GPU (klstm_ctc_beam_decode; kaldi-lstm_amd/csrc/klstm_ctc_beam.hip) against its numpy twin
(tests/ctc_beam_ref.py).  Every integer -- hypotheses, lengths, list sizes, edit distances, all six totals -- must EQUAL the twin; the
probabilities behind a score are bit-identical by construction (one float32 product or sum per step, power-of-two rescale), so the
score may differ by the device's double log and one rounding only: 2 float32 ulps."""
import numpy as np
import pytest

from tests import ctc_beam_ref as Bm
from tests import ctc_decode_ref as D
from tests.nbest_ref import ulps
from tests.test_ctc_beam import (GRID_SEEDS, all_prefixes, exhaustive_case, grid_case, margin, score_excess, softmax_rows)

pytestmark = pytest.mark.gpu


def to_dev(y, window=None):
    """y [T, S, K] -> [T*S, K] float32 CUDA tensor; window = (offset, stride): a column window of a wider matrix full of NaN"""
    import torch
    T, S, K = y.shape
    flat = torch.from_numpy(np.ascontiguousarray(y.reshape(T * S, K)))
    if window is None:
        return flat.cuda()
    off, stride = window
    big = torch.full((T * S, stride), float("nan"), device="cuda")
    big[:, off:off + K] = flat.cuda()
    return big[:, off:off + K]


def run(y, lens, blank, B, C, N, w=None, refs=None, window=None):
    import torch
    import kaldi_lstm_amd as k
    wd = torch.from_numpy(np.asarray(w, np.float32)).cuda() if w is not None else None
    tot = torch.zeros(6, dtype=torch.float64, device="cuda") if refs is not None else None
    res = k.ctc_beam_decode(to_dev(y, window), lens, blank=blank, beam=B, cands=C, nbest=N, class_weight=wd, refs=refs, totals=tot)
    torch.cuda.synchronize()
    return res, (tot.cpu().numpy().tolist() if tot is not None else None)


def check(res, totals, tw, N):
    cnt = res.nbest_count.cpu().numpy().tolist()
    assert cnt == tw["nbest_count"]
    h, n, sc = res.hyp.cpu().numpy(), res.hyp_len.cpu().numpy(), res.score.cpu().numpy()
    worst = (0, (0, 0, 0.0, 0.0))
    for s in range(len(cnt)):
        for q in range(cnt[s]):
            assert n[s, q] == len(tw["hyp"][s][q]) and h[s, q, :n[s, q]].tolist() == tw["hyp"][s][q], (s, q)
            worst = max(worst, (ulps(sc[s, q], tw["score"][s][q]), (s, q, float(sc[s, q]), float(tw["score"][s][q]))))
    assert worst[0] <= 2, worst
    if tw["errors"] is not None:
        assert res.errors.cpu().numpy().tolist() == tw["errors"]
        assert totals == [float(v) for v in tw["totals"]]
    return worst[0]


def run_and_check(y, lens, blank, B, C, N, w=None, refs=None, window=None):
    res, tot = run(y, lens, blank, B, C, N, w, refs, window)
    tw = Bm.beam_twin(y, lens, blank, B, C, N, w=w, refs=refs)
    check(res, tot, tw, N)
    return res, tw


def score_bits(res):
    return res.score.cpu().numpy().view(np.int32)


def ragged_lens(rng, S, T):
    lens = rng.randint(1, T + 1, S).tolist()
    lens[0] = T
    if S >= 4:
        lens[1], lens[2] = 0, 1
    return lens


def make_refs(rng, S, K, blank, longest):
    classes = [c for c in range(K) if c != blank]
    return [[classes[i] for i in rng.randint(0, len(classes), rng.randint(0, longest + 1))] for _ in range(S)]


# ---------------------------------------------------------------------------------------------------------------------------------
# ragged random and peaked posteriors
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "peaked"])
@pytest.mark.parametrize("S,T,K,B,C,N", [(1, 50, 29, 8, 6, 8), (4, 120, 12, 16, 8, 5), (8, 60, 12, 8, 5, 3), (32, 24, 7, 4, 3, 2),
                                         (1, 40, 48, 64, 32, 64), (2, 30, 12, 12, 8, 4)])
def test_ragged_posteriors(kind, S, T, K, B, C, N):
    rng = np.random.RandomState(S * 1000 + T)
    lens = ragged_lens(rng, S, T)
    if kind == "random":
        y = softmax_rows(rng, T, S, K)
        refs = make_refs(rng, S, K, 0, 12)
    else:
        refs = [rng.randint(1, K, max(1, n // 4)).tolist() for n in lens]
        y = D.peaked_case(S + T, T, K, 0, refs, lens, [(s % 2, s % 3 == 0, s % 2, 1) for s in range(S)])
    for s in range(S):
        y[lens[s]:, s] = np.nan                                  # padding rows and idle streams are not read
    run_and_check(y, lens, 0, B, C, N, refs=refs)


@pytest.mark.parametrize("K,B,C,N", [(9, 1, 4, 1), (9, 6, 1, 3), (9, 5, 8, 5), (9, 7, 3, 7), (2, 4, 1, 4), (2, 1, 1, 1)])
def test_edge_parameters(K, B, C, N):
    """B = 1, C = 1, C = K - 1, N = B, K = 2"""
    rng = np.random.RandomState(K * 100 + B * 10 + C)
    S, T = 3, 30
    lens = [30, 17, 1]
    y = softmax_rows(rng, T, S, K, scale=1.0)
    run_and_check(y, lens, K - 1, B, C, N, refs=make_refs(rng, S, K, K - 1, 8))


# ---------------------------------------------------------------------------------------------------------------------------------
# class counts on both sides of every launch geometry of the row top-C, the blank anywhere, with and without class weights
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("K", [2, 29, 63, 64, 65, 256, 257, 2048, 2049, 4097, 16624, 32768])
def test_class_counts_and_blank_position(K, where, weights):
    rng = np.random.RandomState(K + len(where))
    S, T = 2, 12
    blank = dict(first=0, middle=K // 2, last=K - 1)[where]
    y = softmax_rows(rng, T, S, K, scale=3.0)
    w = (0.5 + rng.rand(K)).astype(np.float32) if weights else None
    B, C = 4, min(K - 1, 3)
    run_and_check(y, [T, 7], blank, B, C, 4, w=w, refs=make_refs(rng, S, K, blank, 5))


def test_many_rows_take_the_wave_per_row_geometry():
    """K > 2048 with 4096 rows and more: a wave per row instead of a workgroup per row.  Short utterances keep the twin cheap."""
    rng = np.random.RandomState(11)
    S, T, K = 32, 128, 2100
    lens = [3] * S
    lens[0], lens[31] = 6, 0
    y = np.full((T, S, K), np.nan, np.float32)
    y[:6] = softmax_rows(rng, 6, S, K, scale=3.0)
    run_and_check(y, lens, 5, 4, 3, 2, refs=make_refs(rng, S, K, 5, 3))


def test_column_window_with_odd_offset():
    rng = np.random.RandomState(5)
    S, T, K = 3, 20, 37
    y = softmax_rows(rng, T, S, K)
    w = (0.5 + rng.rand(K)).astype(np.float32)
    for off, stride in ((1, 41), (3, 64), (2, 39)):
        run_and_check(y, [20, 11, 0], 4, 6, 5, 3, w=w, refs=make_refs(rng, S, K, 4, 6), window=(off, stride))


# ---------------------------------------------------------------------------------------------------------------------------------
# planted ties.  Dyadic posteriors: every product and sum is exact, so equal totals are EQUAL and the order alone decides
# ---------------------------------------------------------------------------------------------------------------------------------
def test_planted_ties():
    T = 8
    y = np.zeros((T, 3, 4), np.float32)
    y[:, 0] = 0.25                                                # equal emissions across columns: the lower column ranks first;
    y[:, 1] = [0.5, 0.125, 0.125, 0.25]                           # equal totals across entries: the earlier list position wins
    y[:, 2] = [0.5, 0.25, 0.125, 0.125]
    for B, C in ((4, 3), (3, 2), (8, 3), (2, 1)):
        run_and_check(y, [T, T, T], 0, B, C, B, refs=[[1, 2], [3], [1, 1]])
    # equal PRODUCTS from different factors: 0.25 * 2 = 0.125 * 4 = 0.125 * 4
    w = np.array([1.0, 2.0, 4.0, 4.0], np.float32)
    res, tw = run_and_check(y, [T, T, T], 0, 4, 3, 4, w=w, refs=[[1, 2], [3], [1, 1]])
    assert Bm.candidates(Bm.emissions(y[0, 2], w), 0, 3) == [1, 2, 3]


# ---------------------------------------------------------------------------------------------------------------------------------
# a prefix that leaves the beam and comes back while its extension survives (identity by hash, not by tree node): K = 5, B = 16
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [20, 0, 8, 32, 44])
def test_merge_path(seed):
    y, K, T, B, C = grid_case(seed)
    assert K == 5 and C == 4
    res, tw = run_and_check(y, [T], 0, 16, C, 16)
    hy = [tuple(h) for h in tw["hyp"][0]]
    assert len(set(hy)) == len(hy)


# ---------------------------------------------------------------------------------------------------------------------------------
# zeros and flushes
# ---------------------------------------------------------------------------------------------------------------------------------
def test_nan_inf_tiny_emissions_and_a_dead_utterance():
    rng = np.random.RandomState(9)
    S, T, K = 4, 16, 9
    y = softmax_rows(rng, T, S, K)
    y[2, 0, 3] = np.nan; y[3, 0, 0] = np.nan; y[5, 0, 1] = np.inf; y[6, 0, 2] = -np.inf; y[7, 0, 0] = np.inf
    y[4, 1] = 2.0 ** -61; y[4, 1, 2] = 2.0 ** -60; y[9, 1] *= np.float32(2.0 ** -50)      # below the flush, on it, small but alive
    y[3, 2] = np.nan                                              # an all-NaN row: stream 2 dies
    y[6, 3] = 0.0; y[6, 3, 0] = 1.0                               # only the blank is left
    w = np.ones(K, np.float32)
    w[4] = 2.0 ** -40
    refs = make_refs(rng, S, K, 0, 5)
    for ww in (None, w):
        res, tw = run_and_check(y, [T] * S, 0, 6, 4, 6, w=ww, refs=refs)
        assert tw["nbest_count"][2] == 1 and tw["score"][2] == [-np.inf]
        assert res.score.cpu().numpy()[2, 0] == -np.inf


def test_padding_rows_and_idle_streams_do_not_matter():
    rng = np.random.RandomState(10)
    S, T, K = 5, 20, 300
    lens = [20, 0, 7, 21, 13]
    y = softmax_rows(rng, T, S, K, scale=3.0)
    refs = make_refs(rng, S, K, 0, 5)
    a = y.copy()
    for s in range(S):
        a[lens[s] if 0 < lens[s] <= T else 0:, s] = np.nan
    b = np.where(np.isnan(a), np.float32(7.0), a)
    ra, _ = run_and_check(a, lens, 0, 8, 5, 4, refs=refs)
    rb, _ = run(b, lens, 0, 8, 5, 4, refs=refs)
    cnt = ra.nbest_count.cpu().numpy()
    assert cnt.tolist() == rb.nbest_count.cpu().numpy().tolist() and cnt[1] == 0 and cnt[3] == 0
    for s in range(S):
        for q in range(cnt[s]):
            n = int(ra.hyp_len[s, q])
            assert n == int(rb.hyp_len[s, q]) and ra.hyp[s, q, :n].tolist() == rb.hyp[s, q, :n].tolist()
            assert score_bits(ra)[s, q] == score_bits(rb)[s, q]
    assert ra.errors.tolist() == rb.errors.tolist()


def test_list_shorter_than_nbest():
    import torch
    import kaldi_lstm_amd as k
    rng = np.random.RandomState(12)
    y = softmax_rows(rng, 6, 2, 5)
    y[:, 0, 2:] = 0.0                                             # two live classes: the beam stays small at first
    res = k.ctc_beam_decode(to_dev(y), [1, 0], beam=8, cands=4, nbest=8)
    torch.cuda.synchronize()
    assert res.nbest_count.tolist() == [2, 0]                     # one frame: the empty prefix and [1]


# ---------------------------------------------------------------------------------------------------------------------------------
# the row limit
# ---------------------------------------------------------------------------------------------------------------------------------
def test_row_limit_one_long_stream():
    rng = np.random.RandomState(13)
    y = rng.rand(65535, 1, 4).astype(np.float32)
    res, tw = run_and_check(y, [65535], 0, 2, 1, 2, refs=[[1, 2, 3, 1]])
    assert tw["nbest_count"] == [2] and len(tw["hyp"][0][0]) > 10000


def test_row_limit_many_streams():
    rng = np.random.RandomState(14)
    S, T = 32, 2047
    lens = [int(v) for v in rng.randint(0, 40, S)]
    lens[0], lens[31], lens[7] = T, T, T + 1
    y = np.full((T, S, 4), np.nan, np.float32)
    for s in range(S):
        if 0 < lens[s] <= T:
            y[:lens[s], s] = rng.rand(lens[s], 4).astype(np.float32)
    run_and_check(y, lens, 3, 2, 1, 2, refs=make_refs(rng, S, 4, 3, 20))


# ---------------------------------------------------------------------------------------------------------------------------------
# determinism
# ---------------------------------------------------------------------------------------------------------------------------------
def test_bit_identical_across_runs_and_stream_permutations():
    rng = np.random.RandomState(15)
    S, T, K = 8, 40, 29
    lens = ragged_lens(rng, S, T)
    y = softmax_rows(rng, T, S, K)
    refs = make_refs(rng, S, K, 0, 10)
    ra, ta = run(y, lens, 0, 16, 8, 6, refs=refs)
    rb, tb = run(y, lens, 0, 16, 8, 6, refs=refs)
    perm = rng.permutation(S)
    rc, tc = run(y[:, perm], [lens[p] for p in perm], 0, 16, 8, 6, refs=[refs[p] for p in perm])
    assert ta == tb == tc
    cnt = ra.nbest_count.cpu().numpy()
    assert cnt.tolist() == rb.nbest_count.tolist() and cnt[perm].tolist() == rc.nbest_count.tolist()
    for s2, s in enumerate(perm):
        for q in range(cnt[s]):
            n = int(ra.hyp_len[s, q])
            for r, sx in ((rb, s), (rc, s2)):
                assert int(r.hyp_len[sx, q]) == n and r.hyp[sx, q, :n].tolist() == ra.hyp[s, q, :n].tolist()
                assert score_bits(r)[sx, q] == score_bits(ra)[s, q]
                assert int(r.errors[sx, q]) == int(ra.errors[s, q])


# ---------------------------------------------------------------------------------------------------------------------------------
# statuses and refused limits
# ---------------------------------------------------------------------------------------------------------------------------------
def test_stream_statuses():
    rng = np.random.RandomState(16)
    S, T, K = 6, 14, 7
    y = softmax_rows(rng, T, S, K)
    lens = [14, 0, 9, 14, 15, -3]
    refs = [[1, 2, 3], [1], [], [1, 7, 2], [1], [2]]             # stream 3: a label outside [0, K)
    res, tw = run_and_check(y, lens, 0, 4, 3, 3, refs=refs)
    assert res.nbest_count.tolist() == [3, 0, 3, 3, 0, 0]
    assert res.errors[1].tolist() == [-1] * 3 and res.errors[3].tolist() == [-1] * 3 and res.errors[4].tolist() == [-1] * 3
    res, tw = run_and_check(y, lens, 0, 4, 3, 3, refs=[[1, 2, 3], [1], [], [1, 0, 2], [1] * 1024, [2]])       # the blank as a label
    long_ref = [[1] * 1024] + refs[1:]
    res, tw = run_and_check(y, lens, 0, 4, 3, 3, refs=long_ref)                                         # more than 1023 labels
    assert res.errors[0].tolist() == [-1] * 3 and res.nbest_count[0] == 3
    ok_ref = [[1, 2] * 511 + [3]] + refs[1:]                                                           # 1023: the limit itself
    run_and_check(y, lens, 0, 4, 3, 3, refs=ok_ref)


def test_limits_are_refused_one_step_beyond():
    import torch
    import kaldi_lstm_amd as k

    def refused(T, S, K, B, C, N):
        y = torch.zeros(T * S, K, device="cuda")
        with pytest.raises(k.KlstmError) as ei:
            k.ctc_beam_decode(y, [1] * S, beam=B, cands=C, nbest=N)
        assert ei.value.status == 2, (T, S, K, B, C, N)
    refused(2, 33, 8, 4, 4, 1)               # S <= 32
    refused(65536, 1, 4, 2, 1, 1)            # T * S <= 65535
    refused(2048, 32, 4, 2, 1, 1)
    refused(2, 2, 32769, 4, 4, 1)            # K <= 32768
    refused(2, 2, 8, 65, 4, 1)               # beam <= 64
    refused(2, 2, 64, 4, 33, 1)              # cands <= 32
    refused(2, 2, 8, 4, 8, 1)                # cands <= K - 1
    refused(2, 2, 8, 4, 4, 5)                # nbest <= beam
    y = torch.zeros(4, 1, device="cuda")     # K >= 2
    with pytest.raises(k.KlstmError):
        k.ctc_beam_decode(y, [1, 1], beam=1, cands=1, nbest=1)
    # the limits themselves are served
    rng = np.random.RandomState(17)
    run_and_check(softmax_rows(rng, 3, 32, 40), [3, 2] + [1] * 30, 0, 64, 32, 64)
    run_and_check(softmax_rows(rng, 2, 1, 32768, scale=4.0), [2], 0, 4, 32, 4)


# ---------------------------------------------------------------------------------------------------------------------------------
# the float64 yardsticks: the score is a lower bound of log p(hyp | y), and exact where nothing is pruned
# ---------------------------------------------------------------------------------------------------------------------------------
def test_device_score_is_a_lower_bound_of_the_exact_label_probability():
    """bar: 10 x the largest excess of the NUMPY TWIN on the same inputs (profiles/ctc_beam_parity_margins.json; measured on the twin:
    3.8e-8 relative)"""
    worst = -np.inf
    for seed in GRID_SEEDS:
        y, K, T, B, C = grid_case(seed)
        res, _ = run(y, [T], 0, B, C, B)
        n = int(res.nbest_count[0])
        h, hl, sc = res.hyp.cpu().numpy()[0], res.hyp_len.cpu().numpy()[0], res.score.cpu().numpy()[0]
        dev = dict(hyp=[[h[q, :hl[q]].tolist() for q in range(n)]], score=[[sc[q] for q in range(n)]])
        worst = max(worst, score_excess(y, dev))
    print("largest relative excess of the device's score over the exact log p:", worst)
    assert worst <= margin("lower_bound_rel")


def test_device_exhaustive_beam_gives_exact_label_probabilities():
    """T <= 5, K = 3, B = 64, C = 2: nothing is pruned.  bar: 10 x the twin's largest deviation (measured on the twin: 4.3e-7 relative)"""
    worst = 0.0
    for seed, T in enumerate((1, 2, 3, 4, 5, 5, 5, 5)):
        y = exhaustive_case(seed, T)
        res, tw = run_and_check(y, [T], 0, 64, 2, 64)
        e64 = Bm.emissions64(y[:, 0])
        exact = {tuple(p): Bm.label_logp64(e64, 0, p) for p in all_prefixes(T)}
        n = int(res.nbest_count[0])
        h, hl, sc = res.hyp.cpu().numpy()[0], res.hyp_len.cpu().numpy()[0], res.score.cpu().numpy()[0]
        assert n == sum(v > -np.inf for v in exact.values())
        for q in range(n):
            ex = exact[tuple(h[q, :hl[q]].tolist())]
            worst = max(worst, abs(float(sc[q]) - ex) / abs(ex))
    print("largest relative deviation of the device's exhaustive scores from the exact log p:", worst)
    assert worst <= margin("exhaustive_rel")


def test_nbest_to_lists():
    import kaldi_lstm_amd as k
    rng = np.random.RandomState(18)
    y = softmax_rows(rng, 10, 3, 6)
    refs = [[1, 2], [3], [4]]
    res, _ = run(y, [10, 0, 4], 0, 4, 3, 3, refs=refs)
    tw = Bm.beam_twin(y, [10, 0, 4], 0, 4, 3, 3, refs=refs)
    lists = k.nbest_to_lists(res)
    assert [len(l) for l in lists] == tw["nbest_count"]
    for s, l in enumerate(lists):
        assert [h for h, _, _ in l] == tw["hyp"][s] and [e for _, _, e in l] == tw["errors"][s][:len(l)]


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end through the C++ classes (include/klstm_nnet.hpp CtcBeamDecoder, DecodeCtcWholeUtterances; tests/cpp/ctc_beam_test)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["blstm", "lstm"])
def test_cpp_train_then_beam_decode(tmp_path, kind):
    """The pattern task of the sibling tests, trained with TrainCtcWholeUtterances, then decoded with beam 8, 5 candidates, 4-best:
    the 1-best token error rate is 0, the oracle rate cannot exceed it, beam = 0 leaves the greedy loop as it was, and the minibatch
    the driver dumped gives the same lists through Python and through the twin."""
    from tests.test_ctc_beam import run_driver
    dump = str(tmp_path / "dump.bin")
    r = run_driver("train", kind, dump)
    kv = dict(f.split("=") for f in r.stdout.split() if "=" in f)
    print(f"ctc_beam_test train {kind}:", r.stdout.strip(), flush=True)
    ter, oracle, cv = float(kv["ter_beam"]), float(kv["oracle_beam"]), float(kv["ter_crossvalidate"])
    assert ter == 0.0
    assert oracle <= ter
    assert int(kv["beam0_same"]) == 1 and int(kv["best1_same"]) == 1 and int(kv["lists_ok"]) == 1
    assert int(kv["skipped"]) == 1 and int(kv["scored"]) == 12 and int(kv["cv_scored"]) == 12
    assert cv == ter and float(kv["oracle_crossvalidate"]) == oracle
    assert int(kv["oracle_errors"]) == round(oracle * int(kv["ref_tokens"]))
    raw = np.fromfile(dump, dtype=np.int32)
    T, S, K, N = (int(v) for v in raw[:4])
    p = 4
    lens = raw[p:p + S].tolist(); p += S
    post = raw[p:p + T * S * K].view(np.float32).reshape(T, S, K).copy(); p += T * S * K
    cnt = raw[p:p + S].tolist(); p += S
    hlen = raw[p:p + S * N].reshape(S, N); p += S * N
    score = raw[p:p + S * N].view(np.float32).reshape(S, N); p += S * N
    hyp = raw[p:p + S * N * T].reshape(S, N, T)
    res, tw = run_and_check(post, lens, 0, 8, 5, N)
    assert cnt == tw["nbest_count"]
    for s in range(S):
        for q in range(cnt[s]):
            assert hyp[s, q, :hlen[s, q]].tolist() == tw["hyp"][s][q]
            assert score[s, q].view(np.int32) == res.score.cpu().numpy()[s, q].view(np.int32)
