"""klstm_ctc_nbest_rescore on the device (kaldi_lstm_amd.ctc_nbest_rescore) against its numpy twin (tests/ctc_rescore_ref.py, pinned by a
brute force in tests/test_ctc_rescore.py), at the smallest shapes at which each mechanism can go wrong.

BARS.  order, live_count, units, oov and the re-ranked list's tokens, lengths, counts and errors: equal.  score, add_logp, sub_logp and
out_score: within ONE float32 ulp of the twin's float32 -- the mantissa and the exponent of every walk carry the twin's bits, so both
sides round doubles that differ by the one log (<= 1 ulp of a double) and at most four double operations behind it; they can differ
only where the double lies on a rounding boundary, and then by one ulp: the argument of tests/test_ctc_consensus_gpu.py.  totals: 1e-12
relative (they are sums of integers).
CONDITION every case asserts on its own inputs, from the twin: adjacent ranked z of a stream differ by at least 1e-9 relative, so that
no rank hangs on the last bits of the log, except in the constructed exact tie.
MEASURED on an MI355X: 0 ulps in score, add_logp, sub_logp and out_score in every case, the totals exact
(profiles/ctc_rescore_parity_margins.json).
The conditions on the cases themselves (back-off depths 0 to 3 in the order-4 case, a changed 1-best, an unknown word) are held on the
host first, in tests/test_ctc_rescore.py."""
import numpy as np
import pytest
import torch

from tests import ctc_consensus_ref as C
from tests import ctc_rescore_ref as R
from tests.margins import bound
from tests.nbest_ref import garbage, ulps

pytestmark = pytest.mark.gpu
GAP = 1e-9
_DEV = {}


def dev_model(model, blank):
    """one device blob per model of the session"""
    import kaldi_lstm_amd as k
    key = (id(model), blank)
    if key not in _DEV:
        _DEV[key] = (model, k.CtcSparseLabelLm(model, blank))
    return _DEV[key][1]


def twin_of(case):
    w = case.get("words")
    return R.rescore(case["hyp"], case["hyp_len"], case["count"], case["logp"], case["K"], sub=case.get("sub"), add=case.get("add"),
                     words=R.Words(*w) if w else None, add_reserved=case.get("add_blank", 0) if w else -1,
                     am_scale=case.get("am_scale", 1.0), add_scale=case.get("add_scale", 1.0), unit_bonus=case.get("unit_bonus", 0.0),
                     errors=case.get("errors"), max_len=case.get("max_len"), out_n=case.get("out_n"), out_stride=case.get("out_stride"))


def device(case, want_totals=True, stream=None):
    import kaldi_lstm_amd as k
    t = {n: torch.from_numpy(np.ascontiguousarray(case[n])).cuda() for n in ("hyp", "hyp_len", "count", "logp")}
    errors = torch.from_numpy(case["errors"]).cuda() if case.get("errors") is not None else None
    totals = torch.zeros(8, dtype=torch.float64, device="cuda") if want_totals else None
    w = case.get("words")
    r = k.ctc_nbest_rescore((t["hyp"], t["hyp_len"], t["count"], errors), logp=t["logp"], classes=case["K"],
                            sub=dev_model(case["sub"], 0) if case.get("sub") is not None else None,
                            add=dev_model(case["add"], case.get("add_blank", 0)) if case.get("add") is not None else None,
                            words=k.CtcWordTable(*w) if w else None, am_scale=case.get("am_scale", 1.0),
                            add_scale=case.get("add_scale", 1.0), unit_bonus=case.get("unit_bonus", 0.0), out_n=case.get("out_n"),
                            out_stride=case.get("out_stride"), max_len=case.get("max_len"), totals=totals, stream=stream)
    if stream is not None:
        stream.synchronize()
    out = {n: r[n].cpu().numpy() for n in ("order", "live_count", "score", "add_logp", "sub_logp", "units", "oov")}
    nb = r["nbest"]
    if nb is not None:
        out.update(out_hyp=nb.hyp.cpu().numpy(), out_len=nb.hyp_len.cpu().numpy(), out_count=nb.nbest_count.cpu().numpy(),
                   out_score=nb.score.cpu().numpy(), out_errors=nb.errors.cpu().numpy() if nb.errors is not None else None)
    out["totals"] = totals.cpu().numpy() if want_totals else None
    out["result"] = r
    return out


def check(case):
    case = garbage(case)
    o = twin_of(case)
    gap = R.min_gap(o, skip=case.get("tie_streams", ()))
    assert gap >= GAP, gap
    d = device(case)
    ints = ["order", "live_count", "units", "oov"]
    flts = ["score", "add_logp", "sub_logp"]
    if d.get("out_hyp") is not None:
        ints += ["out_hyp", "out_len", "out_count"] + (["out_errors"] if case.get("errors") is not None else [])
        flts += ["out_score"]
    for n in ints:
        assert np.array_equal(d[n], o[n]), (n, d[n], o[n])
    for n in flts:
        bound(ulps(d[n], o[n]), 1, f"{n} (float32 ulps)")
    t = o["totals"]
    bound(float((np.abs(d["totals"] - t) / np.maximum(np.abs(t), 1.0)).max()), 1e-12, "totals (relative)")
    return d, o


@pytest.fixture(scope="module")
def models():
    corpus, bigram, order4 = R.token_models()
    return dict(corpus=corpus, bigram=bigram, order4=order4, bigram_nofinal=bigram._replace(final=None),
                order4_nofinal=order4._replace(final=None))


@pytest.fixture(scope="module")
def wordset():
    return R.word_setup()


# ------------------------------------------------------------------------------------------------------------------------------------
# 1, 2: token level
# ------------------------------------------------------------------------------------------------------------------------------------
def test_tiny(models):
    """lengths 0, 1 and 2; an empty hypothesis (only the final weight applies); stream 2: two identical entries of equal logp"""
    hyp = np.array([[[0, 0], [5, 0]], [[1, 2], [1, 0]], [[3, 0], [3, 0]]], np.int32)
    hyp_len = np.array([[0, 1], [2, 1], [1, 1]], np.int32)
    logp = np.array([[-0.5, -1.25], [-2.0, -0.75], [-1.5, -1.5]], np.float32)
    case = dict(hyp=hyp, hyp_len=hyp_len, count=np.array([2, 2, 2], np.int32), logp=logp, K=12, add=models["bigram"], tie_streams=(2,))
    d, o = check(case)
    assert d["order"][2].tolist() == [0, 1] and d["score"][2, 0] == d["score"][2, 1]
    fin0 = np.float64(R.flush(models["bigram"].final[0]))
    assert d["units"][0].tolist() == [0, 1] and abs(float(d["add_logp"][0, 0]) - np.log(fin0)) <= 1e-6


@pytest.mark.parametrize("final", [True, False])
@pytest.mark.parametrize("which", ["bigram", "order4"])
def test_token_level_add_only(models, which, final):
    model = models[which if final else which + "_nofinal"]
    hyp, hyp_len, count, logp = R.lists_from_corpus(1, models["corpus"], 4, 8, 12)
    d, o = check(dict(hyp=hyp, hyp_len=hyp_len, count=count, logp=logp, K=12, add=model, add_scale=0.7, unit_bonus=0.3))
    assert (d["live_count"] == 8).all()
    assert 8 <= hyp_len.mean() <= 16


# ------------------------------------------------------------------------------------------------------------------------------------
# 3: sub + add on the lists of the search
# ------------------------------------------------------------------------------------------------------------------------------------
def test_sub_and_add_on_the_lists_of_the_search(models):
    import kaldi_lstm_amd as k
    from tests import ctc_mbr_ref as M
    T, K, lens = 40, 12, [40, 33, 27, 40]
    refs = [models["corpus"][i][:9] for i in (0, 5, 11, 17)]
    y = M.peaked(3, T, K, lens, refs, sigma=1.2, bump=2.5).reshape(T * 4, K).cuda()
    first = dev_model(models["bigram"], 0)
    nb = k.ctc_beam_decode(y, lens, beam=16, cands=8, nbest=8, refs=refs, lm=first)
    case = dict(hyp=nb.hyp.cpu().numpy(), hyp_len=nb.hyp_len.cpu().numpy(), count=nb.nbest_count.cpu().numpy(), logp=nb.score.cpu().numpy(),
                errors=nb.errors.cpu().numpy(), K=K, sub=models["bigram"], add=models["order4"])
    assert (case["count"] >= 2).all()
    totals = torch.zeros(8, dtype=torch.float64, device="cuda")
    r = k.ctc_nbest_rescore(nb, add=dev_model(models["order4"], 0), sub=first, totals=totals)
    o = twin_of(garbage(case))
    assert R.min_gap(o) >= GAP
    for n in ("order", "live_count", "units", "oov"):
        assert np.array_equal(r[n].cpu().numpy(), o[n]), n
    for n in ("score", "add_logp", "sub_logp"):
        bound(ulps(r[n].cpu().numpy(), o[n]), 1, f"{n} (float32 ulps)")
    assert np.array_equal(r["nbest"].errors.cpu().numpy(), o["out_errors"]) and np.array_equal(r["nbest"].hyp_len.cpu().numpy(), o["out_len"])
    t = totals.cpu().numpy()
    bound(float((np.abs(t - o["totals"]) / np.maximum(np.abs(o["totals"]), 1.0)).max()), 1e-12, "totals (relative)")
    assert t[0] == 4 and t[5] == case["errors"][:, 0].sum()
    lists = k.nbest_to_lists(r)                                      # the dict stands for its list
    assert [h for h, _, _ in lists[0]] == [case["hyp"][0, q, :case["hyp_len"][0, q]].tolist() for q in o["order"][0, :o["live_count"][0]]]
    # identity: what was taken out is put back in
    same = k.ctc_nbest_rescore(nb, add=first, sub=first)
    cnt = case["count"]
    for s in range(4):
        assert same["order"][s].cpu().tolist() == list(range(cnt[s])) + [-1] * (8 - cnt[s])
        bound(ulps(same["score"][s, :cnt[s]].cpu().numpy(), case["logp"][s, :cnt[s]]), 1, "identity score against logp (float32 ulps)")


# ------------------------------------------------------------------------------------------------------------------------------------
# 4: word mode
# ------------------------------------------------------------------------------------------------------------------------------------
def word_case(ws, keys=None, ids=None, unk=None, **kw):
    hyp, hyp_len, count, logp = R.word_lists(ws)
    k0, i0 = ws["table"]
    return dict(hyp=hyp, hyp_len=hyp_len, count=count, logp=logp, K=ws["K"], add=ws["model"], add_blank=ws["reserved"],
                words=(k0 if keys is None else keys, i0 if ids is None else ids, ws["unk"] if unk is None else unk, ws["sep"]), **kw)


def test_words(wordset):
    d, o = check(word_case(wordset, add_scale=0.8, unit_bonus=0.5))
    assert d["oov"].sum() >= 1 and d["totals"][7] == d["oov"].sum() and d["units"][1, 5] == 0
    assert (d["live_count"] == 8).all()                              # an unknown word takes its class


def test_words_unknown_forbids(wordset):
    d, o = check(word_case(wordset, unk=-1))
    assert d["totals"][3] >= 1 and d["totals"][3] == (d["oov"] > 0).sum()
    assert np.isinf(d["score"][d["oov"] > 0]).all()


def test_words_table_ids_out_of_range_and_reserved(wordset):
    keys, ids = wordset["table"]
    ids = ids.copy()
    used = list(dict.fromkeys(wordset["sents"][0] + wordset["sents"][1]))[:3]          # three words that occur in the lists
    rows = [int(np.flatnonzero(ids == w)[0]) for w in used]
    ids[rows[0]], ids[rows[1]], ids[rows[2]] = wordset["V"], wordset["reserved"], -5
    d, o = check(word_case(wordset, ids=ids))
    plain = twin_of(garbage(word_case(wordset)))
    assert d["oov"].sum() > plain["oov"].sum()


def test_words_unsorted_table(wordset):
    """no fault, and the bits of the twin's bisection on the same unsorted arrays: misses only"""
    keys, ids = wordset["table"]
    perm = np.random.default_rng(1).permutation(len(keys))
    d, o = check(word_case(wordset, keys=keys[perm], ids=ids[perm]))
    plain = twin_of(garbage(word_case(wordset)))
    assert d["oov"].sum() > plain["oov"].sum()


# ------------------------------------------------------------------------------------------------------------------------------------
# 5: capacity
# ------------------------------------------------------------------------------------------------------------------------------------
def test_capacity_tokens(models):
    """max_len 1023: entries of exactly 1023 tokens, of 1024 (dropped) and of 1020"""
    rng = np.random.default_rng(5)
    base = rng.integers(1, 12, size=1024)
    hyp = np.zeros((1, 3, 1024), np.int32)
    hyp[0, 0, :1023], hyp[0, 1], hyp[0, 2, :1020] = base[:1023], base, np.delete(base[:1023], [7, 500, 1000])
    case = dict(hyp=hyp, hyp_len=np.array([[1023, 1024, 1020]], np.int32), count=np.array([3], np.int32),
                logp=np.array([[-1.0, -0.5, -2.0]], np.float32), K=12, add=models["order4"], sub=models["bigram"], max_len=1023)
    d, o = check(case)
    assert d["units"][0].tolist() == [1023, 0, 1020] and d["totals"][2] == 1 and np.isinf(d["score"][0, 1]) and d["live_count"][0] == 2


def test_capacity_words(wordset):
    """1023 tokens alternating token and separator: 512 words of one token"""
    rng = np.random.default_rng(6)
    hyp = np.zeros((1, 2, 1023), np.int32)
    hyp[0, 0, 0::2] = rng.integers(1, wordset["K"], size=512)
    hyp[0, 1, 0::2] = rng.integers(1, wordset["K"], size=512)
    k0, i0 = wordset["table"]
    case = dict(hyp=hyp, hyp_len=np.array([[1023, 1023]], np.int32), count=np.array([2], np.int32), logp=np.array([[-1.0, -1.5]], np.float32),
                K=wordset["K"], add=wordset["model"], add_blank=wordset["reserved"], words=(k0, i0, wordset["unk"], wordset["sep"]),
                max_len=1023)
    d, o = check(case)
    assert d["units"][0].tolist() == [512, 512] and 0 < d["oov"][0, 0] < 512


# ------------------------------------------------------------------------------------------------------------------------------------
# 6, 7: ragged lists, forbidding
# ------------------------------------------------------------------------------------------------------------------------------------
def case_ragged(models):
    hyp, hyp_len, count, logp = R.lists_from_corpus(4, models["corpus"], 6, 8, 12, stride=24)
    count = np.array([8, 0, 3, 1, 8, 9], np.int32)
    logp[0, 1], logp[0, 2], logp[0, 3] = -np.inf, np.nan, np.inf
    hyp_len[0, 4], hyp_len[0, 5] = -1, 25
    hyp[4, 2, 3], hyp[4, 5, 0] = -2, 12
    errors = np.random.default_rng(9).integers(0, 6, size=(6, 8)).astype(np.int32)
    return dict(hyp=hyp, hyp_len=hyp_len, count=count, logp=logp, K=12, add=models["order4"], sub=models["bigram"], errors=errors)


def test_ragged(models):
    d, o = check(case_ragged(models))
    assert d["live_count"].tolist() == [3, 0, 3, 1, 6, 0] and d["totals"][:3].tolist() == [4, 2, 7]
    assert (d["order"][[1, 5]] == -1).all() and np.isinf(d["score"][[1, 5]]).all()


def test_forbidding():
    rows = [[[1, 1], [2], [1, 2], [3], [1], []],                     # fine, zero arc weight, miss without back-off, next outside, zero final, fine
            [[2], [1, 2], [3], [1], [1, 1, 1], [2, 2]]]              # all forbidden: the stream is idle
    hyp, hyp_len, count = R.pack(rows)
    logp = np.array([[-1, -0.5, -0.25, -0.125, -0.0625, -3], [-1, -2, -3, -4, -5, -6]], np.float32)
    d, o = check(dict(hyp=hyp, hyp_len=hyp_len, count=count, logp=logp, K=4, add=R.forbidding_model()))
    assert d["order"][0].tolist() == [0, 5, -1, -1, -1, -1] and d["live_count"].tolist() == [2, 0]
    assert d["totals"].tolist() == [1, 1, 0, 10, 0, 0, 0, 0] and o["status"] == ["done", "idle"]
    assert np.isinf(d["add_logp"][0, 1:5]).all() and abs(float(d["add_logp"][0, 5]) - np.log(0.5)) <= 1e-6


# ------------------------------------------------------------------------------------------------------------------------------------
# 8: the re-ranked list, into the consensus
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_n", [1, 3, 8])
def test_list_outputs_feed_the_consensus(models, out_n):
    import kaldi_lstm_amd as k
    case = dict(case_ragged(models), out_n=out_n, out_stride=31)
    d, o = check(case)
    assert d["out_hyp"].shape == (6, out_n, 31) and d["out_count"].tolist() == np.minimum(o["live_count"], out_n).tolist()
    r = k.ctc_nbest_consensus(d["result"], want_dist=True)
    # the twin's list with the device's scores (held to one ulp of the twin's above): the consensus of that list
    oc = C.consensus(o["out_hyp"], o["out_len"], o["out_count"], d["out_score"])
    for n in ("pick", "map", "mbr", "unit_len", "dist"):
        assert np.array_equal(getattr(r, n).cpu().numpy(), oc[n]), n
    for n in ("post", "risk"):
        a, b = getattr(r, n).cpu().numpy(), oc[n]
        assert np.array_equal(a < 0, b < 0)
        bound(ulps(np.abs(a), np.abs(b)), 1, f"consensus {n} (float32 ulps)")


# ------------------------------------------------------------------------------------------------------------------------------------
# 10: through the C++ classes (include/klstm_nnet.hpp CtcRescorer, CtcWordTable, DecodeCtcOptions::rescorer; tests/cpp/ctc_rescore_test)
# ------------------------------------------------------------------------------------------------------------------------------------
class Dump:
    def __init__(self, path):
        self.raw, self.p = np.fromfile(path, dtype=np.int32), 0

    def ints(self, n):
        v = self.raw[self.p:self.p + n].copy()
        self.p += n
        return v

    def one(self):
        return int(self.ints(1)[0])

    def floats(self, n):
        return self.ints(n).view(np.float32)

    def model(self):
        import kaldi_lstm_amd as k
        Q, A, classes, blank = (int(v) for v in self.ints(4))
        off, lab, nxt, wt = self.ints(Q + 1), self.ints(A), self.ints(A), self.floats(A)
        return k.SparseLm(classes, off, lab, nxt, wt, self.ints(Q), self.floats(Q), self.floats(Q)), blank


def test_cpp_rescorer_behind_the_beam_decoder(tmp_path):
    """The pattern task trained for a few epochs only, so that the lists differ.  DecodeCtcWholeUtterances without a rescorer (what it
    reported before: the heads of the lists, the new statistics zero), with one that puts back what it takes out (the same answers),
    and with a token-level one and a consensus behind it; a word-level CtcRescorer of the driver's own on the same minibatches.  The
    driver dumps its models, its table and per minibatch the search's device arrays with both rescorers' outputs: Python's call on the
    same arrays writes the same bits, and both lie within the bars of the twin."""
    import kaldi_lstm_amd as k
    from tests.test_ctc_rescore import run_driver
    path = str(tmp_path / "dump.bin")
    r = run_driver("run", 12, path)
    print("ctc_rescore_test:", r.stdout.strip(), flush=True)
    kv = dict(f.split("=") for f in r.stdout.split() if "=" in f)
    for flag in ("off_zero", "heads", "identity_same", "lists_match", "heads_tok", "conf_ok", "rates_ok", "has_report"):
        assert int(kv[flag]) == 1, flag
    assert int(kv["minibatches"]) == 2 and int(kv["tok_utts"]) == 8 and int(kv["wrd_utts"]) == 8
    d = Dump(path)
    K = d.one()
    (sub, _), (add, _), (word, reserved) = d.model(), d.model(), d.model()
    W = d.one()
    keys, ids, unk, sep = d.ints(2 * W).view(np.uint64), d.ints(W), d.one(), d.one()
    assert np.array_equal(keys, np.sort(keys)) and sorted(int(x) for x in keys) == sorted(k.word_key(w) for w in ([2], [3], [2, 3], [4, 5]))
    dsub, dadd, dword = k.CtcSparseLabelLm(sub, 0), k.CtcSparseLabelLm(add, 0), k.CtcSparseLabelLm(word, reserved)
    table = k.CtcWordTable(keys, ids, unk, sep)
    passes = (dict(add=add, dadd=dadd, words=None, add_scale=0.8, unit_bonus=0.25),
              dict(add=word, dadd=dword, words=(keys, ids, unk, sep), add_scale=0.5, unit_bonus=0.0))
    first_errors = new_errors = changed = oov = 0
    for _ in range(2):
        T, S, N = d.one(), d.one(), d.one()
        cnt, hlen, score, err = d.ints(S), d.ints(S * N).reshape(S, N), d.floats(S * N).reshape(S, N), d.ints(S * N).reshape(S, N)
        hyp = d.ints(S * N * T).reshape(S, N, T)
        case = garbage(dict(hyp=hyp, hyp_len=hlen, count=cnt, logp=score, errors=err, K=K, sub=sub))
        t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (hyp, hlen, cnt, err, score)]
        for i, ps in enumerate(passes):
            cpp = dict(order=d.ints(S * N).reshape(S, N), live_count=d.ints(S), score=d.floats(S * N).reshape(S, N),
                       add_logp=d.floats(S * N).reshape(S, N), sub_logp=d.floats(S * N).reshape(S, N), units=d.ints(S * N).reshape(S, N),
                       oov=d.ints(S * N).reshape(S, N), out_count=d.ints(S), out_len=d.ints(S * N).reshape(S, N),
                       out_score=d.floats(S * N).reshape(S, N), out_errors=d.ints(S * N).reshape(S, N), out_hyp=d.ints(S * N * T).reshape(S, N, T))
            py = k.ctc_nbest_rescore((t[0], t[1], t[2], t[3]), logp=t[4], classes=K, sub=dsub, add=ps["dadd"], words=table if ps["words"] else None,
                                     add_scale=ps["add_scale"], unit_bonus=ps["unit_bonus"], out_stride=T)
            o = twin_of(dict(case, add=ps["add"], words=ps["words"], add_blank=reserved, add_scale=ps["add_scale"], unit_bonus=ps["unit_bonus"],
                             out_stride=T))
            assert R.min_gap(o) >= GAP
            for n in ("order", "live_count", "score", "add_logp", "sub_logp", "units", "oov"):       # the bits of Python's call
                assert cpp[n].tobytes() == py[n].cpu().numpy().tobytes(), n
            nb = py["nbest"]
            assert np.array_equal(cpp["out_count"], nb.nbest_count.cpu().numpy()) and np.array_equal(cpp["out_count"], o["out_count"])
            for s in range(S):
                c = int(cpp["out_count"][s])
                assert cpp["out_len"][s, :c].tobytes() == nb.hyp_len[s, :c].cpu().numpy().tobytes() == o["out_len"][s, :c].tobytes()
                assert cpp["out_score"][s, :c].tobytes() == nb.score[s, :c].cpu().numpy().tobytes()
                assert np.array_equal(cpp["out_errors"][s, :c], o["out_errors"][s, :c])
                for q in range(c):
                    assert np.array_equal(cpp["out_hyp"][s, q, :cpp["out_len"][s, q]], o["out_hyp"][s, q, :o["out_len"][s, q]])
            for n in ("order", "live_count", "units", "oov"):
                assert np.array_equal(cpp[n], o[n]), n
            for n in ("score", "add_logp", "sub_logp"):
                bound(ulps(cpp[n], o[n]), 1, f"C++ {n} (float32 ulps)")
            if i == 0:
                first_errors, new_errors, changed = first_errors + o["totals"][5], new_errors + o["totals"][6], changed + o["totals"][4]
            else:
                oov += o["totals"][7]
    assert d.p == d.raw.size
    assert float(kv["tok_first_errors"]) == first_errors and float(kv["tok_rescored_errors"]) == new_errors
    assert float(kv["changed"]) == changed and int(kv["wrd_oov"]) == oov


# ------------------------------------------------------------------------------------------------------------------------------------
# 9: determinism and size
# ------------------------------------------------------------------------------------------------------------------------------------
def test_bit_reproducible_and_stream_permutation(models):
    case = garbage(case_ragged(models))
    a, b = device(case), device(case)
    names = [n for n in a if n not in ("result",) and a[n] is not None]
    for n in names:
        assert a[n].tobytes() == b[n].tobytes(), n
    perm = np.array([4, 2, 5, 0, 3, 1])
    p = device(dict(case, **{n: case[n][perm] for n in ("hyp", "hyp_len", "count", "logp", "errors")}))
    for n in names:
        if n != "totals":
            assert p[n].tobytes() == a[n][perm].tobytes(), n
    assert np.array_equal(p["totals"], a["totals"])                  # sums of integers: any order


def test_maximum_shape(models):
    hyp, hyp_len, count, logp = R.lists_from_corpus(2, models["corpus"], 32, 64, 12, spread=40.0)
    d, o = check(dict(hyp=hyp, hyp_len=hyp_len, count=count, logp=logp, K=12, add=models["order4"], sub=models["bigram"]))
    assert (d["live_count"] == 64).all()


def test_short_workspace_is_an_error_and_writes_nothing(models):
    import ctypes
    import kaldi_lstm_amd as k
    lib = k.load_library()
    hyp, hyp_len, count, logp = R.lists_from_corpus(1, models["corpus"], 3, 8, 12)
    S, N, stride = hyp.shape
    t = [torch.from_numpy(a).cuda() for a in (hyp, hyp_len, count, logp)]
    m = dev_model(models["bigram"], 0)
    need = k.ctc_rescore_workspace_bytes(S, N, stride)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    outs = [torch.full((S * N,), -77, dtype=torch.int32, device="cuda") for _ in range(3)]
    totals = torch.full((8,), -77.0, dtype=torch.float64, device="cuda")

    def call(nbytes):
        return lib.klstm_ctc_nbest_rescore(t[0].data_ptr(), stride, t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), None, S, N, stride, 12,
                                           None, ctypes.c_size_t(0), 0, None, m.blob.data_ptr(), ctypes.c_size_t(m.nbytes), m.states, 12,
                                           m.final.data_ptr(), None, None, 0, -1, -1, -1, 1.0, 1.0, 0.0, outs[0].data_ptr(), outs[1].data_ptr(),
                                           outs[2].data_ptr(), None, None, None, None, 0, None, 0, None, None, None, None, totals.data_ptr(),
                                           ws.data_ptr(), ctypes.c_size_t(nbytes), None)
    assert call(need - 1) == 1 and lib.klstm_last_error().startswith(b"klstm_ctc_nbest_rescore: workspace")
    torch.cuda.synchronize()
    assert all((o == -77).all() for o in outs) and (totals == -77).all()
    assert call(need) == 0
    torch.cuda.synchronize()
    assert (outs[1][:S] == N).all() and totals[0] == -77 + S
