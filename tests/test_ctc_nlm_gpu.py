"""The knlm_* entries and CtcNeuralLm on the device (include/klstm_nlm.h; kaldi_lstm_amd.nlm) against the numpy twin
(tests/ctc_nlm_ref.py, pinned by a brute force in tests/test_ctc_nlm.py), at the smallest shapes that exercise every edge of the plan:
S = 3, N = 3 and E = 4 (three groups, the last with one live stream), max_len = 7 with T = 3 (three chunks, the last partial, the end
term of a 6-token entry alone in its chunk), K = 6.

BARS.  knlm_pack, knlm_rank: bit for bit (the rank is fed the twin's accumulators).  knlm_score_rows on given float32 logits against
float64: |acc - float64| <= BAR_ROWS * norm per entry, norm = max(positions, |float64 acc|) -- every lp is <= 0, so |acc| is the sum of
the |lp| and norm is the number of positions with every position weighted by max(1, |lp|) up to a factor of two: the scale on which a
float32 value of lp has its ulp.  BAR_ROWS is 10 x the largest error measured on an MI355X (profiles/ctc_nlm_parity_margins.json).
WHY A NORM: the regimes the issue sets reach |lp| = 160 a position, where one float32 ulp of lp is 1.5e-5, next to |lp| of about 1; an
absolute bar fitted to the former would not see an error a hundred times too large in the latter.  Where |lp| <= 1 the norm is the
number of positions and the bar is absolute.
End to end: per entry |acc(GPU) - float64 twin| <= max(3 |float32 twin - float64 twin|, BAR_ROWS * positions scored), the
engine-versus-oracle convention with the floor the issue sets; the order is compared only after the float64 twin's adjacent ranked
z have been found more than 100 x that bar apart.
MEASURED on an MI355X (profiles/ctc_nlm_parity_margins.json): knlm_score_rows 3.0e-8 (V = 7), 3.9e-8 (V = 65), 2.3e-8 (V = 2052) against the
bar of 4e-7; end to end between 0.24 and 0.60 of the bar; pack, rank, the C++ rescorer and a stream of its own: the same bits."""
import numpy as np
import pytest
import torch

from tests import ctc_nlm_ref as R
from tests.margins import bound

pytestmark = pytest.mark.gpu
BAR_ROWS = 4e-7          # 10 x the 3.93e-8 measured over the widths 7, 65, 2052 and the regimes (the largest: V = 65, the N(0, 25) rows)
K = 6


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_lists(hyp, hyp_len, count, logp, errors=None):
    return (dev(hyp), dev(hyp_len), dev(count), dev(errors) if errors is not None else None), dev(logp)


def dev_lm(lm, E=4, T=3):
    import kaldi_lstm_amd as k
    return k.CtcNeuralLm(lm.layers, lm.W, lm.b, embed=lm.embed, bos=lm.bos, eos=lm.eos, num_stream=E, chunk=T, classes=K)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def norm_of(acc64, positions):
    return np.maximum(np.maximum(positions, 1), np.abs(np.where(np.isfinite(acc64), acc64, 0.0)))


# ------------------------------------------------------------------------------------------------------------------------------------
# knlm_pack
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["onehot", "embedding"])
def test_pack_is_the_twins_rows(form):
    import kaldi_lstm_amd as k
    lm = R.make_lm(K, 7, 6, 6, D=8 if form == "embedding" else None)
    hyp, hyp_len, count, logp, _ = R.poisoned_lists(K=K, max_len=7)
    lists, lp = dev_lists(hyp, hyp_len, count, logp)
    embed = (dev(lm.embed[0]), dev(lm.embed[1])) if lm.embed is not None else None
    cols, E, T = (8 if embed else 7), 4, 3
    seen = 0
    for first in (0, 4, 8):
        for t0 in (0, 3, 6):
            buf = torch.full((T * E, cols + 3), 777.0, device="cuda")
            k.knlm_pack(lists, K, 7, lm.bos, lm.eos, first, E, T, t0, buf[:, :cols], embed, logp=lp, max_len=7)
            got = buf.cpu().numpy()
            want = R.pack_rows(hyp, hyp_len, count, logp, K, lm, first, E, T, t0, max_len=7)
            assert np.array_equal(bits(got[:, :cols]), bits(want)), (first, t0)
            assert (got[:, cols:] == 777.0).all(), "columns beyond the row were written"
            seen += int((np.abs(want).sum(1) > 0).sum())
    assert seen == 1 + 8 + 4 + 6 + 6 + 7                               # every position of every well-formed entry, once


# ------------------------------------------------------------------------------------------------------------------------------------
# knlm_score_rows on given logits
# ------------------------------------------------------------------------------------------------------------------------------------
def rows_case(V, seed=0):
    """S = 2, N = 3, max_len = 7, eos = V - 1; six well-formed entries, one per regime: N(0, 1) rows; rows at +-80; the target 100 below
    the row's maximum; a NaN in the row of position 1; N(0, 25) rows; an empty hypothesis.  -> lists, logits [group][9 * 4, V], the
    float64 accumulators, positions"""
    rng = np.random.RandomState(seed + V)
    lens = [7, 5, 7, 3, 6, 0]
    hyp = np.full((2, 3, 8), 10 ** 6, np.int32)
    for se, n in enumerate(lens):
        hyp[se // 3, se % 3, :n] = rng.randint(0, K, size=n)
    hyp_len, count, logp = np.array(lens, np.int32).reshape(2, 3), np.array([3, 3], np.int32), -np.ones((2, 3), np.float32)
    E, P, eos = 4, 9, V - 1
    logits = [rng.randn(P * E, V).astype(np.float32) for _ in range(2)]
    ref, pos = np.zeros(6), np.zeros(6, np.int32)
    for se, n in enumerate(lens):
        a, e = logits[se // E], se % E
        tg = R.targets_of(hyp[se // 3, se % 3, :n].tolist(), eos)
        for p, t in enumerate(tg):
            row = a[p * E + e]
            if se == 1:
                row[:] = 80.0 * np.sign(row) + rng.randn(V).astype(np.float32)
            if se == 2:
                row[t] = np.delete(row, t).max() - 100.0
            if se == 3 and p == 1:
                row[rng.randint(0, V)] = np.nan
            if se == 4:
                row *= 5.0
            ref[se] += R.row_logp64(row, t)
        pos[se] = len(tg)
    return (hyp, hyp_len, count, logp), logits, ref, pos


@pytest.mark.parametrize("V", [7, 65, 2052])
def test_score_rows_against_float64(V):
    import kaldi_lstm_amd as k
    (hyp, hyp_len, count, logp), logits, ref, pos = rows_case(V)
    lists, lp = dev_lists(hyp, hyp_len, count, logp)
    E, eos = 4, V - 1

    def run(T):
        acc = torch.full((6,), 123.0, dtype=torch.float64, device="cuda")          # the chunk with t0 == 0 sets, it does not add
        n = torch.full((6,), 55, dtype=torch.int32, device="cuda")
        for g, a in enumerate(logits):
            buf = torch.full((a.shape[0], V + 1), np.nan, device="cuda")           # rows V + 1 floats apart: no row but the first is 16-byte aligned
            buf[:, :V] = dev(a)
            for t0 in range(0, 9, T):
                k.knlm_score_rows(buf[t0 * E:(t0 + T) * E, :V], lists, K, eos, g * E, E, T, t0, acc, n, logp=lp, max_len=7)
        return acc.cpu().numpy(), n.cpu().numpy()
    acc3, n3 = run(3)
    acc9, n9 = run(9)
    assert np.array_equal(n3, pos) and np.array_equal(n9, pos)
    assert np.array_equal(bits(acc3), bits(acc9)), "three chunks and one chunk must add the same values in the same order"
    assert not np.isfinite(acc3[3]) and not np.isfinite(ref[3])                      # the NaN row
    fin = np.arange(6) != 3
    assert np.isfinite(acc3[fin]).all() and ref[2] < -100.0 * pos[2]
    err = np.abs(acc3[fin] - ref[fin]) / norm_of(ref, pos)[fin]
    print(f"knlm_score_rows V={V}: |acc - float64| / norm per entry = {err}", flush=True)
    bound(float(err.max()), BAR_ROWS, f"|acc - float64| / norm, V = {V}")


# ------------------------------------------------------------------------------------------------------------------------------------
# knlm_rank fed the twin's accumulators
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_n", [3, 2, 0])
def test_rank_is_the_twins(out_n):
    import kaldi_lstm_amd as k
    lm = R.make_lm(K, K, 0, 0)
    hyp, hyp_len, count, logp, errors = R.poisoned_lists(K=K, max_len=7, more_streams=True)
    acc, _, _ = R.score_entries(hyp, hyp_len, count, logp, K, lm, 7)
    acc[1, 1] = -np.inf                                                 # a forbidden entry; stream 1 is left without a live one
    acc[np.asarray(R.well_formed(hyp, hyp_len, count, logp, K, 7)) != 3] = np.nan   # what belongs to no well-formed entry is not looked at
    kw = dict(am_scale=0.9, nlm_scale=0.7, unit_bonus=0.3)
    o = R.rank(hyp, hyp_len, count, logp, K, acc, True, errors=errors, max_len=7, out_n=out_n, **kw)
    assert o["status"] == ["done", "idle", "done", "idle", "rejected"] and o["totals"][3] == 1
    lists, lp = dev_lists(hyp, hyp_len, count, logp, errors)
    S, N, stride = hyp.shape
    start = np.arange(8) * 1.5 + 2.0
    totals = dev(start.copy())
    out = None
    if out_n:
        out = k.CtcBeamResult(torch.full((S, out_n, 7), -9, dtype=torch.int32, device="cuda"), torch.full((S, out_n), -9, dtype=torch.int32, device="cuda"),
                              torch.full((S,), -9, dtype=torch.int32, device="cuda"), torch.full((S, out_n), -9.0, device="cuda"),
                              torch.full((S, out_n), -9, dtype=torch.int32, device="cuda"))
    r = k.knlm_rank(lists, K, dev(acc), True, out_n=out_n, logp=lp, max_len=7, out=out, totals=totals, **kw)
    for name in ("order", "live_count", "units"):
        assert np.array_equal(getattr(r, name).cpu().numpy(), o[name]), name
    for name in ("score", "nlm_logp"):
        assert np.array_equal(bits(getattr(r, name).cpu().numpy()), bits(o[name])), name
    assert np.array_equal(totals.cpu().numpy(), start + o["totals"])                # integers onto halves: exact
    if not out_n:
        assert r.nbest is None
        return
    oh, ol, oc, osc, oe = (t.cpu().numpy() for t in r.nbest)
    assert np.array_equal(oc, o["out_count"])
    for s in range(S):
        for q in range(out_n):
            if q >= oc[s]:                                              # beyond the count: left alone
                assert (oh[s, q] == -9).all() and ol[s, q] == -9 and osc[s, q] == -9.0 and oe[s, q] == -9
                continue
            n = ol[s, q]
            assert n == o["out_len"][s, q] and np.array_equal(oh[s, q, :n], o["out_hyp"][s, q, :n]) and (oh[s, q, n:] == -9).all()
            assert bits(osc[s, q:q + 1]) == bits(o["out_score"][s, q:q + 1]) and oe[s, q] == o["out_errors"][s, q]


# ------------------------------------------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------------------------------------------
LMS = {
    # name: (V, bos = eos, layers, embedding rows)
    "one_layer": (6, 0, 1, None),
    "two_layers": (6, 0, 2, None),
    "one_layer_embedding": (7, 6, 1, 8),
    "two_layers_embedding": (7, 6, 2, 8),
}
SCALES = dict(am_scale=1.0, nlm_scale=0.8, unit_bonus=0.4)
_SEARCH = {}


def search_lists(seed=2):
    """the lists ctc_beam_decode itself finds on peaked posteriors: T = 7 frames (the stride, so max_len = 7), S = 3, N = 3; computed once"""
    import kaldi_lstm_amd as k
    from tests import ctc_mbr_ref as M
    if seed not in _SEARCH:
        T, lens, refs = 7, [7, 6, 5], [[1, 2, 3, 5], [4, 5, 1], [2, 2, 1]]
        y = M.peaked(seed, T, K, lens, refs, sigma=1.5, bump=2.0).reshape(T * 3, K).cuda()
        nb = k.ctc_beam_decode(y, lens, beam=8, cands=4, nbest=3, refs=refs)
        _SEARCH[seed] = (nb, tuple(t.cpu().numpy() for t in (nb.hyp, nb.hyp_len, nb.nbest_count, nb.score, nb.errors)))
    return _SEARCH[seed]


def entry_bars(lm, host, o64):
    """per entry max(3 |float32 twin - float64 twin|, BAR_ROWS * positions scored)"""
    hyp, hyp_len, count, logp, _ = host
    a32, _, _ = R.score_entries(hyp, hyp_len, count, logp, K, lm, 7, dtype=np.float32)
    return np.maximum(3.0 * np.abs(a32 - o64["acc"]), BAR_ROWS * np.maximum(o64["positions"], 1))


def check_acc(r, o64, bars, what):
    acc = r.acc.cpu().numpy()
    assert np.array_equal(r.positions.cpu().numpy(), o64["positions"])
    frac = np.abs(acc - o64["acc"]) / bars
    print(f"{what}: |acc - float64 twin| / bar per entry, largest {frac.max():.3g}; bars {bars.min():.3g} .. {bars.max():.3g}", flush=True)
    bound(float(frac.max()), 1.0, f"{what}: |nlm_logp - float64 twin| as a fraction of max(3 |float32 twin - float64 twin|, floor)")
    live = np.isfinite(o64["score"])
    nl = r.nlm_logp.cpu().numpy()
    assert np.array_equal(bits(nl[live]), bits(acc[live].astype(np.float32))) and (nl[~live] == -np.inf).all()
    return acc


def check_order(r, o64, bars, totals=None):
    gap = R.min_gap(o64)
    assert gap > 100.0 * bars.max(), (gap, bars.max())                 # held on the CPU first: no rank hangs on what the bar allows
    for name in ("order", "live_count", "units"):
        assert np.array_equal(getattr(r, name).cpu().numpy(), o64[name]), name
    oh, ol, oc, _, oe = (t.cpu().numpy() for t in r.nbest)
    assert np.array_equal(oc, o64["out_count"]) and np.array_equal(ol, o64["out_len"]) and np.array_equal(oh, o64["out_hyp"])
    assert np.array_equal(oe, o64["out_errors"])
    sc = r.nbest.score.cpu().numpy()
    listed = np.arange(sc.shape[1])[None, :] < oc[:, None]
    assert (np.abs(sc[listed] - o64["out_score"][listed]) <= 2.0 * bars.max() + 1e-6 * np.abs(sc[listed])).all()
    if totals is not None:
        assert np.array_equal(totals.cpu().numpy(), o64["totals"])      # integers


@pytest.mark.parametrize("name", sorted(LMS))
def test_rescore_on_the_lists_of_the_search(name):
    V, b, n_lstm, D = LMS[name]
    lm = R.make_lm(K, V, b, b, n_lstm=n_lstm, D=D)
    nb, host = search_lists()
    hyp, hyp_len, count, logp, errors = host
    assert hyp.shape == (3, 3, 7) and (count >= 2).all()
    o64 = R.rescore(hyp, hyp_len, count, logp, K, lm, max_len=7, errors=errors, **SCALES)
    bars = entry_bars(lm, host, o64)
    d = dev_lm(lm)
    totals = torch.zeros(8, dtype=torch.float64, device="cuda")
    r = d.rescore(nb, totals=totals, **SCALES)
    check_acc(r, o64, bars, name)
    check_order(r, o64, bars, totals)
    r2 = d.rescore(nb, **SCALES)                                         # the same call again: the same bits
    for a, c in zip(r[:5] + tuple(r.nbest) + (r.acc,), r2[:5] + tuple(r2.nbest) + (r2.acc,)):
        assert torch.equal(a, c)
    d.close()


def test_rescore_on_the_poisoned_lists():
    """every edge of the plan on the twin's terms: dropped entries inside a group, the end term of the 6-token entry 8 alone in the last
    chunk of the last group.  The accumulators only: streams 2's equal entries run in different engine streams"""
    lm = R.make_lm(K, 7, 6, 6, n_lstm=1, D=8)
    host = R.poisoned_lists(K=K, max_len=7)
    hyp, hyp_len, count, logp, errors = host
    o64 = R.rescore(hyp, hyp_len, count, logp, K, lm, max_len=7, errors=errors)
    lists, lp = dev_lists(hyp, hyp_len, count, logp, errors)
    d = dev_lm(lm)
    r = d.rescore(lists, logp=lp, max_len=7)
    check_acc(r, o64, entry_bars(lm, host, o64), "poisoned lists")
    assert np.array_equal(r.live_count.cpu().numpy(), o64["live_count"]) and np.array_equal(r.units.cpu().numpy(), o64["units"])
    d.close()


def test_result_does_not_depend_on_streams_and_chunk():
    lm = R.make_lm(K, 6, 0, 0, n_lstm=2)
    nb, host = search_lists()
    hyp, hyp_len, count, logp, errors = host
    o64 = R.rescore(hyp, hyp_len, count, logp, K, lm, max_len=7, errors=errors, **SCALES)
    bars = entry_bars(lm, host, o64)
    for E in (4, 8):
        for T in (3, 20):
            d = dev_lm(lm, E, T)
            r = d.rescore(nb, **SCALES)
            check_acc(r, o64, bars, f"E = {E}, T = {T}")
            check_order(r, o64, bars)
            d.close()


def test_a_stream_of_its_own_gives_the_same_bits():
    """CtcNeuralLm(stream=...): the engines and every launch of the pass on one explicit stream, ordered with the caller's"""
    import kaldi_lstm_amd as k
    lm = R.make_lm(K, 7, 6, 6, n_lstm=2, D=8)
    nb, _ = search_lists()
    d = dev_lm(lm)
    want = d.rescore(nb, **SCALES)
    own = k.CtcNeuralLm(lm.layers, lm.W, lm.b, embed=lm.embed, bos=lm.bos, eos=lm.eos, num_stream=4, chunk=3, classes=K, stream=torch.cuda.Stream())
    got = own.rescore(nb, **SCALES)
    for a, c in zip(want[:5] + tuple(want.nbest) + (want.acc, want.positions), got[:5] + tuple(got.nbest) + (got.acc, got.positions)):
        assert torch.equal(a, c)
    # a busy caller: products queued on the current stream in front of the call, so that the fills of the outputs (which the call
    # enqueues there) run long after the own stream could have started -- the pass must wait for them, and what the caller enqueues
    # next must wait for the pass
    big = torch.randn(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    for _ in range(3):
        for _ in range(20):
            big = (big @ big) * 1e-2
        got = own.rescore(nb, **SCALES)
        copies = [t.clone() for t in got[:5] + tuple(got.nbest) + (got.acc, got.positions)]      # on the caller's stream, no synchronise in between
        for a, c in zip(want[:5] + tuple(want.nbest) + (want.acc, want.positions), copies):
            assert torch.equal(a, c)
    for m in (d, own):
        m.close()


def test_staging_behind_the_ngram_second_pass_and_before_the_consensus():
    import kaldi_lstm_amd as k
    from tests import ctc_rescore_ref as G
    corpus = G.token_corpus(7, K, n=40, L=6)
    bigram = k.backoff_ngram_label_lm(corpus, K, 0, order=2)
    nb, _ = search_lists()
    first = k.ctc_nbest_rescore(nb, add=k.CtcSparseLabelLm(bigram, 0), add_scale=0.5)
    mid = first["nbest"]
    host = tuple(t.cpu().numpy() for t in (mid.hyp, mid.hyp_len, mid.nbest_count, mid.score, mid.errors))
    lm = R.make_lm(K, 6, 0, 0)
    o64 = R.rescore(*host[:4], K, lm, max_len=7, errors=host[4], **SCALES)
    bars = entry_bars(lm, host, o64)
    d = dev_lm(lm)
    r = d.rescore(first, **SCALES)                                       # the dict of the n-gram stage stands for its list
    check_acc(r, o64, bars, "behind ctc_nbest_rescore")
    check_order(r, o64, bars)
    c = k.ctc_nbest_consensus(r, scale=1.0)                              # ... and this stage's result for its own
    pick = c.pick.cpu().numpy()
    assert ((pick >= 0) & (pick < r.nbest.nbest_count.cpu().numpy())).all()
    assert k.nbest_to_lists(r)[0][0][0] == host[0][0, o64["order"][0, 0], :host[1][0, o64["order"][0, 0]]].tolist()
    d.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# the pieces meet: a trained LM moves the lawful entry up
# ------------------------------------------------------------------------------------------------------------------------------------
def test_a_trained_lm_prefers_the_lawful_entry():
    """the toy language next = previous % 7 + 1 over the tokens 1 .. 7 (V = 8, the blank 0 is bos and eos): a one-layer LM (C = 32,
    R = 16, 4 streams) trained for 300 minibatches by the existing trainer pieces (DataParallelNnet over LstmDP, AffineDP and
    SoftmaxXentDP) on lm_training_utterances; then lists whose first entry breaks the rule once and whose second obeys it, 0.2 apart"""
    import kaldi_lstm_amd as k
    from tests.nnet_twins import make_stack
    V, C, Rr, S, T = 8, 32, 16, 4, 8
    lstm, W, b = make_stack((V, C, Rr, 1, V), S, seed=5, dtype=np.float32, scale=0.1)
    e = k.Engine(V, C, Rr, S)
    e.set_params(lstm[0])
    aff = k.AffineDP(dev(W), dev(b), k)
    net = k.DataParallelNnet([k.LstmDP(e), aff], k.SoftmaxXentDP(k, lazy=True), alloc=lambda n: torch.zeros(n, device="cuda"))
    rng = np.random.RandomState(1)
    for _ in range(300):
        seqs = []
        for s in range(S):
            c, y = int(rng.randint(1, 8)), []
            for _ in range(int(rng.randint(3, 8))):
                y.append(c)
                c = c % 7 + 1
            seqs.append(y)
        x, tg, mk = np.zeros((T * S, V), np.float32), np.zeros(T * S, np.int32), np.zeros(T * S, np.float32)
        for s, (f, t) in enumerate(k.lm_training_utterances(seqs, V, 0, 0)):
            rows = np.arange(len(t)) * S + s
            x[rows], tg[rows], mk[rows] = f, t, 1
        net.train_step(dev(x), dev(tg), dev(mk), 0.9, 0.01, reset_flags=[1] * S)
    e.synchronize()
    hyp = np.zeros((2, 2, 8), np.int32)
    hyp[0, 0, :6], hyp[0, 1, :6] = [3, 4, 6, 6, 7, 1], [3, 4, 5, 6, 7, 1]
    hyp[1, 0, :4], hyp[1, 1, :4] = [7, 1, 1, 3], [7, 1, 2, 3]
    hyp_len, count = np.array([[6, 6], [4, 4]], np.int32), np.array([2, 2], np.int32)
    logp = np.array([[-1.0, -1.2], [-2.0, -2.2]], np.float32)
    lists, lp = dev_lists(hyp, hyp_len, count, logp)
    trained = k.CtcNeuralLm([(e.get_params(), V, C, Rr)], aff.W.cpu().numpy(), aff.bias.cpu().numpy(), bos=0, eos=0, num_stream=4, chunk=8)
    r = trained.rescore(lists, logp=lp, max_len=8)
    nl = r.nlm_logp.cpu().numpy()
    print("trained LM: nlm_logp", nl.tolist(), flush=True)
    assert r.order.cpu().numpy().tolist() == [[1, 0], [1, 0]] and (nl[:, 1] > nl[:, 0] + 2.0).all()
    blank_lm = k.CtcNeuralLm([(np.zeros_like(lstm[0]), V, C, Rr)], np.zeros_like(W), np.zeros_like(b), bos=0, eos=0, num_stream=4, chunk=8)
    r0 = blank_lm.rescore(lists, logp=lp, max_len=8)
    assert r0.order.cpu().numpy().tolist() == [[0, 1], [0, 1]]          # every position costs log 8 in both entries: the order stays
    assert np.allclose(r0.nlm_logp.cpu().numpy(), -np.log(8.0) * np.array([[7, 7], [5, 5]]), rtol=1e-6)
    for m in (trained, blank_lm):
        m.close()
    e.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# the C++ side: tests/cpp/ctc_nlm_test.cpp
# ------------------------------------------------------------------------------------------------------------------------------------
def run_driver(*args):
    from tests import cpp_driver
    return cpp_driver.run("ctc_nlm_test", *args, timeout=300, headers=cpp_driver.HEADERS + ("klstm_nlm.h",))


def test_cpp_rescorer_gives_the_bits_of_the_python_call(tmp_path):
    """CtcNeuralRescorer on a model file written by Nnet::Write (embedding, an LstmProjectedStreams and an LstmProjected layer, Affine,
    Softmax): the same engines and kernels in the same order as CtcNeuralLm.rescore, so the same bits"""
    from tests import kaldi_fmt
    lm = R.make_lm(K, 7, 6, 6, n_lstm=2, D=8)
    nb, host = search_lists()
    hyp, hyp_len, count, logp, errors = host
    S, N, stride = hyp.shape
    (f0, i0, c0, r0), (f1, i1, c1, r1) = lm.layers
    model = kaldi_fmt.nnet_binary([("affine", lm.embed[0], lm.embed[1]), ("lstm_streams", f0, i0, c0, r0, 4), ("lstm", f1, i1, c1, r1),
                                   ("affine", lm.W, lm.b), ("softmax", 7)])
    (tmp_path / "lm.nnet").write_bytes(model)
    with open(tmp_path / "lists.bin", "wb") as fh:
        fh.write(np.array([S, N, stride], np.int32).tobytes())
        for a in (count, hyp_len, logp, errors, hyp):
            fh.write(np.ascontiguousarray(a).tobytes())
    r = run_driver("rescore", tmp_path / "lm.nnet", tmp_path / "lists.bin", tmp_path / "dump.bin", 4, 3, K, 6, 6, SCALES["am_scale"],
                   SCALES["nlm_scale"], SCALES["unit_bonus"])
    assert "utterances=6 " in r.stdout and "lists=3" in r.stdout, r.stdout                # two calls over three streams
    d = dev_lm(lm)
    py = d.rescore(nb, **SCALES)
    raw = np.fromfile(tmp_path / "dump.bin", np.int32)
    SN, o = S * N, 0
    want = [("order", py.order, SN), ("live", py.live_count, S), ("score", py.score, SN), ("nlm_logp", py.nlm_logp, SN), ("units", py.units, SN),
            ("out count", py.nbest.nbest_count, S), ("out len", py.nbest.hyp_len, SN), ("out score", py.nbest.score, SN),
            ("out errors", py.nbest.errors, SN), ("out hyp", py.nbest.hyp, SN * stride)]
    for name, t, n in want:
        assert np.array_equal(raw[o:o + n], t.cpu().numpy().ravel().view(np.int32)), name
        o += n
    assert o == raw.size
    d.close()


def test_cpp_decode_loop_with_and_without_the_neural_rescorer():
    """DecodeCtcWholeUtterances: without the option what it reports today; with an LM of scale 0 the same answers; behind the n-gram
    rescorer and before the consensus the stages read each other's lists"""
    r = run_driver("decode", 30)
    out = dict(kv.split("=") for kv in r.stdout.split()[1:])
    for key in ("off_zero", "zero_same", "heads", "conf_ok", "staged", "has_report"):
        assert out[key] == "1", (key, r.stdout, r.stderr)
    assert float(out["utterances"]) == 8
