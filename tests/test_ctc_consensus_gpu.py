"""klstm_ctc_consensus on the device (kaldi_lstm_amd.ctc_nbest_consensus) against its numpy twin (tests/ctc_consensus_ref.py, pinned by a
brute force in tests/test_ctc_consensus.py), at the smallest shapes at which each mechanism can go wrong.

BARS.  pick, map, mbr, unit_len and dist: equal.  post, risk, conf: within ONE float32 ulp of the twin's float32 -- both sides round
doubles that agree to ~1e-14 relative (at most 70 double roundings and one exp of <= 1 ulp), so they differ only where the double lies on
a rounding boundary, and then by one ulp.  totals: 1e-12 relative.
CONDITIONS every case asserts on its own inputs, from the twin: a relative gap >= 1e-9 between the two smallest risks and between the
two largest z of every stream (so that no argmin / argmax hangs on the last bits), except in the constructed exact tie; and in every
case drawn from the generator at least one stream where the MBR entry is not the MAP entry.  The generator
(ctc_consensus_ref.make_lists) draws DISTINCT entries per list, as a search returns them: two equal entries have bitwise equal risks.
MEASURED on an MI355X: 0 ulps in post, risk and conf in every case, totals within 2.7e-16 relative (parity_margins.json of the run).
The end-to-end cases take the peaked posteriors of tests/ctc_mbr_ref.py (tests/regimes.py holds parameters and inputs of the LSTM
layer, no posteriors)."""
import numpy as np
import pytest
import torch

from tests import ctc_consensus_ref as C
from tests.margins import bound
from tests.nbest_ref import garbage, ulps

pytestmark = pytest.mark.gpu
GAP = 1e-9


def generated(seed, S, N, L=None, lens=None, stride=None, **kw):
    hyp, hyp_len, count, logp = C.make_lists(seed, S, N, L, lens=lens, stride=stride)
    return dict(hyp=hyp, hyp_len=hyp_len, count=count, logp=logp, **kw)


def case_tiny():
    """lengths 0, 1 and 2, one empty hypothesis; stream 2: equal logp, an exact tie of z and of R that the lowest q wins"""
    hyp = np.array([[[0, 0], [5, 0]], [[1, 2], [1, 0]], [[3, 0], [4, 0]]], np.int32)
    hyp_len = np.array([[0, 1], [2, 1], [1, 1]], np.int32)
    logp = np.array([[-0.5, -1.25], [-2.0, -0.75], [-1.5, -1.5]], np.float32)
    return dict(hyp=hyp, hyp_len=hyp_len, count=np.array([2, 2, 2], np.int32), logp=logp, tie_streams=(2,))


def case_capacity():
    """max_len 1023: one entry of exactly 1023 units, one of 1024 tokens (dropped), one of 1020"""
    rng = np.random.default_rng(5)
    base = rng.integers(1, 30, size=1024)
    hyp = np.zeros((1, 3, 1024), np.int32)
    hyp[0, 0, :1023] = base[:1023]
    hyp[0, 1] = base
    short = np.delete(base[:1023], [7, 500, 1000])
    short[300] = 31
    hyp[0, 2, :1020] = short
    return dict(hyp=hyp, hyp_len=np.array([[1023, 1024, 1020]], np.int32), count=np.array([3], np.int32),
                logp=np.array([[-1.0, -0.5, -2.0]], np.float32), max_len=1023)


def case_ragged(seed=4):
    """counts [8, 0, 3, 1, 8] and a rejected stream (count N + 1); entries dropped for -inf, NaN, +inf, a negative length, a length
    above the stride and a negative token; a stride wider than any length"""
    c = generated(seed, 6, 8, 12, stride=24)
    c["count"] = np.array([8, 0, 3, 1, 8, 9], np.int32)
    c["logp"][0, 1], c["logp"][0, 2], c["logp"][0, 3] = -np.inf, np.nan, np.inf
    c["hyp_len"][0, 4], c["hyp_len"][0, 5] = -1, 25
    c["hyp"][4, 2, 3] = -2
    return c


def case_words(seed=0):
    """about 300 tokens in about 60 words per entry, separator class 0: word-level edits of one base sentence per stream, with leading,
    trailing and doubled separators thrown in, and one entry of separators alone"""
    rng = np.random.default_rng(100 + seed)
    S, N, sep = 2, 8, 0
    rows = []
    for s in range(S):
        base = [rng.integers(1, 6, size=int(rng.integers(3, 6))).tolist() for _ in range(60)]
        ent = []
        for q in range(N):
            words = [list(w) for w in base]
            for _ in range(int(rng.integers(0, 4))):
                kind, pos = int(rng.integers(0, 3)), int(rng.integers(0, len(words)))
                if kind == 0:
                    words[pos] = rng.integers(1, 6, size=3).tolist()
                elif kind == 1:
                    del words[pos]
                else:
                    words.insert(pos, rng.integers(1, 6, size=2).tolist())
            toks = [sep] * int(rng.integers(0, 3))
            for w in words:
                toks += w + [sep] * int(rng.integers(1, 3) if rng.random() < 0.2 else 1)
            if rng.random() < 0.5:
                toks = toks[:-1]                       # no trailing separator
            ent.append(toks)
        rows.append(ent)
    rows[1][5] = [sep] * 4
    stride = max(len(t) for e in rows for t in e) + 3
    hyp, hyp_len = np.zeros((S, N, stride), np.int32), np.zeros((S, N), np.int32)
    for s, ent in enumerate(rows):
        for q, t in enumerate(ent):
            hyp[s, q, :len(t)], hyp_len[s, q] = t, len(t)
    logp = -np.sort(4.0 * rng.random((S, N)), axis=1).astype(np.float32)
    return dict(hyp=hyp, hyp_len=hyp_len, count=np.full(S, N, np.int32), logp=logp, separator=sep)


def device(case, pivot="mbr", want_totals=True, stream=None):
    import kaldi_lstm_amd as k
    dev = "cuda"
    t = {n: torch.from_numpy(np.ascontiguousarray(case[n])).to(dev) for n in ("hyp", "hyp_len", "count", "logp")}
    errors = torch.from_numpy(case["errors"]).to(dev) if case.get("errors") is not None else None
    totals = torch.zeros(10, dtype=torch.float64, device=dev) if want_totals else None
    r = k.ctc_nbest_consensus((t["hyp"], t["hyp_len"], t["count"], errors), logp=t["logp"], scale=case.get("scale", 1.0),
                              separator=case.get("separator"), pivot=pivot, max_len=case.get("max_len"), want_dist=True, totals=totals,
                              stream=stream)
    if stream is not None:
        stream.synchronize()
    out = {n: getattr(r, n).cpu().numpy() for n in r._fields}
    out["totals"] = totals.cpu().numpy() if want_totals else None
    return out


def twin_of(case, pivot="mbr"):
    sep = case.get("separator")
    return C.consensus(case["hyp"], case["hyp_len"], case["count"], case["logp"], scale=case.get("scale", 1.0),
                       separator=-1 if sep is None else sep, pivot_mode=1 if pivot == "mbr" else 0, errors=case.get("errors"),
                       max_len=case.get("max_len"))


def conditions(case, o, need_differ):
    ties = case.get("tie_streams", ())
    keep = [s for s in range(len(o["pick"])) if s not in ties]
    sub = {k: (v[keep] if isinstance(v, np.ndarray) and v.shape[:1] == o["pick"].shape else v) for k, v in o.items()}
    g_r, g_z = C.gaps(sub)
    assert g_r >= GAP and g_z >= GAP, (g_r, g_z)
    if need_differ:
        assert (o["mbr"] != o["map"]).any(), "no stream where the MBR entry is not the MAP entry"


def check(case, pivot="mbr", need_differ=False):
    case = garbage(case)
    o = twin_of(case, pivot)
    conditions(case, o, need_differ)
    d = device(case, pivot)
    for n in ("pick", "map", "mbr", "unit_len", "dist"):
        assert np.array_equal(d[n], o[n]), (n, d[n], o[n])
    for n in ("post", "risk", "conf"):
        bound(ulps(d[n], o[n]), 1, f"{n} (float32 ulps)")
    t = o["totals"]
    bound(float((np.abs(d["totals"] - t) / np.maximum(np.abs(t), 1.0)).max()), 1e-12, "totals (relative)")
    return d, o


def test_tiny():
    d, o = check(case_tiny())
    assert d["pick"].tolist() == [0, 1, 0] and d["unit_len"].tolist() == [[0, 1], [2, 1], [1, 1]]
    assert d["risk"][2, 0] == d["risk"][2, 1] == 0.5
    check(case_tiny(), pivot="map")


def test_lane_boundary():
    """lengths around 63 | 64, where the columns go from one to four per lane; a pivot of 63 and one of 64 units"""
    case = generated(2, 4, 8, lens=[63, 64, 63, 64])
    d, o = check(case, need_differ=True)
    assert case["hyp_len"].min() <= 62 and case["hyp_len"].max() >= 66
    assert {63, 64} <= set(o["unit_len"][np.arange(4), o["pick"]].tolist())


def test_second_boundary():
    case = generated(0, 2, 16, lens=[255, 256])
    d, o = check(case, need_differ=True)
    assert case["hyp_len"].min() <= 254 and case["hyp_len"].max() >= 257


def test_capacity():
    d, o = check(case_capacity())
    assert d["risk"][0].tolist()[1] == -1 and d["unit_len"][0].tolist() == [1023, 0, 1020] and d["totals"][7] == 1
    assert d["dist"][0, 0, 2] == 4


def test_full_list():
    check(generated(0, 2, 64, 40), need_differ=True)


def test_ragged():
    case = case_ragged()
    d, o = check(case, need_differ=True)
    assert d["pick"][[1, 5]].tolist() == [-1, -1] and (d["pick"][[0, 2, 3, 4]] >= 0).all()
    assert (d["post"][0] > 0).tolist() == [True, False, False, False, False, False, True, True]
    assert d["totals"][:2].tolist() == [4, 2] and d["totals"][7] == 6
    assert (d["conf"][3, :d["unit_len"][3, 0]] == 1).all()       # one live entry


def test_words():
    case = case_words()
    d, o = check(case, need_differ=True)
    assert d["unit_len"][1, 5] == 0 and 55 <= d["unit_len"][0, 0] <= 65 and case["hyp_len"].max() >= 250
    tokens = dict(case, separator=None)
    dt, _ = check(tokens)
    assert not np.array_equal(dt["dist"], d["dist"])


@pytest.mark.parametrize("with_errors", [False, True])
@pytest.mark.parametrize("scale", [0.5, 1.0, 3.0])
@pytest.mark.parametrize("pivot", ["map", "mbr"])
def test_pivot_modes_scales_errors(pivot, scale, with_errors):
    case = generated(0, 3, 8, 12, scale=scale)
    if with_errors:
        case["errors"] = np.random.default_rng(9).integers(0, 6, size=(3, 8)).astype(np.int32)
    d, o = check(case, pivot=pivot, need_differ=True)
    assert np.array_equal(d["pick"], d["mbr"] if pivot == "mbr" else d["map"])
    assert (d["totals"][8] > 0) == with_errors


# ------------------------------------------------------------------------------------------------------------------------------------
# end to end: the lists of the search
# ------------------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_from_the_beam_search():
    import kaldi_lstm_amd as k
    from tests import ctc_mbr_ref as M
    T, K, lens = 60, 20, [60, 47, 33]
    refs = M.random_refs(2, K, [14, 11, 8])
    y = M.peaked(2, T, K, lens, refs, sigma=1.2, bump=2.5).reshape(T * 3, K).cuda()
    nb = k.ctc_beam_decode(y, lens, beam=16, cands=8, nbest=8, refs=refs)
    exact = k.ctc_mbr_eval(y, lens, nb).hyp_logp
    for logp in (None, exact):
        totals = torch.zeros(10, dtype=torch.float64, device="cuda")
        r = k.ctc_nbest_consensus(nb, logp=logp, want_dist=True, totals=totals)
        case = dict(hyp=nb.hyp.cpu().numpy(), hyp_len=nb.hyp_len.cpu().numpy(), count=nb.nbest_count.cpu().numpy(),
                    logp=(nb.score if logp is None else logp).cpu().numpy(), errors=nb.errors.cpu().numpy())
        o = twin_of(case)
        conditions(case, o, False)
        for n in ("pick", "map", "mbr", "unit_len", "dist"):
            assert np.array_equal(getattr(r, n).cpu().numpy(), o[n]), n
        for n in ("post", "risk", "conf"):
            bound(ulps(getattr(r, n).cpu().numpy(), o[n]), 1, f"{n} (float32 ulps)")
        bound(float((np.abs(totals.cpu().numpy() - o["totals"]) / np.maximum(np.abs(o["totals"]), 1.0)).max()), 1e-12, "totals (relative)")
        lists = k.consensus_to_lists(r, nb)
        for s, e in enumerate(lists):
            p = int(o["pick"][s])
            assert e["pick"] == p and [u for u, _ in e["units"]] == case["hyp"][s, p, :case["hyp_len"][s, p]].tolist()
            assert ulps([c for _, c in e["units"]], o["conf"][s, :o["conf_len"][s]]) <= 1
            assert abs(e["risk"] - float(o["risk"][s, p])) <= 1e-6 * max(1.0, e["risk"])


def test_end_to_end_words_through_a_lexicon():
    import kaldi_lstm_amd as k
    from kaldi_lstm_amd import lm as LM
    from tests import ctc_mbr_ref as M
    T, K, blank, sep = 80, 8, 0, 1
    words = [[2, 3], [4], [5, 6, 7], [3, 2], [6, 4]]
    sents = [[0, 2, 1, 4, 3], [1, 1, 0, 2]]
    refs = [sum(([*words[w], sep] for w in snt), [])[:-1] for snt in sents]
    lens = [80, 64]
    y = M.peaked(5, T, K, lens, refs, sigma=1.0, bump=2.0).reshape(T * 2, K).cuda()
    lex = k.CtcLabelLm(*LM.lexicon_label_lm(words, K, blank, sep))
    nb = k.ctc_beam_decode(y, lens, beam=16, cands=4, nbest=8, refs=refs, lm=lex)
    r = k.ctc_nbest_consensus(nb, separator=sep, want_dist=True)
    case = dict(hyp=nb.hyp.cpu().numpy(), hyp_len=nb.hyp_len.cpu().numpy(), count=nb.nbest_count.cpu().numpy(), logp=nb.score.cpu().numpy(),
                separator=sep)
    assert (case["count"] >= 2).all()
    o = twin_of(case)
    conditions(case, o, False)
    for n in ("pick", "map", "mbr", "unit_len", "dist"):
        assert np.array_equal(getattr(r, n).cpu().numpy(), o[n]), n
    for n in ("post", "risk", "conf"):
        bound(ulps(getattr(r, n).cpu().numpy(), o[n]), 1, f"{n} (float32 ulps)")
    for s, e in enumerate(k.consensus_to_lists(r, nb, separator=sep)):
        assert all(w in words for w, _ in e["units"]) and len(e["units"]) == o["conf_len"][s]


# ------------------------------------------------------------------------------------------------------------------------------------
# end to end through the C++ classes (include/klstm_nnet.hpp CtcConsensus, DecodeCtcWholeUtterances; tests/cpp/ctc_consensus_test)
# ------------------------------------------------------------------------------------------------------------------------------------
def test_cpp_consensus_behind_the_beam_decoder(tmp_path):
    """The pattern task trained for a few epochs only, so that the lists differ; DecodeCtcWholeUtterances with consensus 0 (what the
    search gives without the option, byte for byte), 1 (the head of every list, with confidences) and 2 (the MBR entry), and a
    CtcConsensus of the driver's own behind the decoder over the two minibatches of the pass, held against the twin on the dumped lists."""
    from tests.test_ctc_consensus import run_driver
    dump = str(tmp_path / "dump.bin")
    r = run_driver("run", 12, dump)
    print("ctc_consensus_test:", r.stdout.strip(), flush=True)
    kv = dict(f.split("=") for f in r.stdout.split() if "=" in f)
    for flag in ("off_same", "map_ok", "mbr_ok", "conf_ok", "search_same", "map_risk_same", "has_report"):
        assert int(kv[flag]) == 1, flag
    assert int(kv["minibatches"]) == 2 and int(kv["own_utts"]) == 8
    assert float(kv["expected_mbr"]) <= float(kv["expected_map"]) and 0 < float(kv["mean_conf_mbr"]) <= 1
    raw = np.fromfile(dump, dtype=np.int32)
    p, tot = 0, np.zeros(10)
    for _ in range(2):
        T, S, N = (int(v) for v in raw[p:p + 3]); p += 3
        cnt = raw[p:p + S].copy(); p += S
        hlen = raw[p:p + S * N].reshape(S, N); p += S * N
        score = raw[p:p + S * N].view(np.float32).reshape(S, N); p += S * N
        err = raw[p:p + S * N].reshape(S, N); p += S * N
        hyp = raw[p:p + S * N * T].reshape(S, N, T); p += S * N * T
        pick, imap, imbr, nconf = (raw[p + i * S:p + (i + 1) * S] for i in range(4)); p += 4 * S
        nflat = int(raw[p]); p += 1
        flat = raw[p:p + nflat].view(np.float32); p += nflat
        risk = raw[p:p + S].view(np.float32); p += S
        case = garbage(dict(hyp=hyp, hyp_len=hlen, count=cnt, logp=score, errors=err))
        o = twin_of(case)
        conditions(case, o, False)
        assert np.array_equal(pick, o["pick"]) and np.array_equal(imap, o["map"]) and np.array_equal(imbr, o["mbr"])
        assert np.array_equal(nconf, o["conf_len"])
        bound(ulps(flat, np.concatenate([o["conf"][s, :o["conf_len"][s]] for s in range(S)])), 1, "conf (float32 ulps)")
        bound(ulps(risk, o["risk"][np.arange(S), o["pick"]]), 1, "risk (float32 ulps)")
        tot += o["totals"]
    assert p == raw.size
    for name, want in (("own_expected", tot[2] / tot[0]), ("own_map_expected", tot[3] / tot[0]), ("own_mean_conf", tot[6] / tot[5]),
                       ("expected_mbr", tot[2] / tot[0])):
        bound(abs(float(kv[name]) - want) / max(abs(want), 1.0), 1e-12, f"{name} (relative)")
    assert int(kv["pick_errors"]) == int(tot[8])


# ------------------------------------------------------------------------------------------------------------------------------------
# robustness
# ------------------------------------------------------------------------------------------------------------------------------------
def test_bit_reproducible_and_on_a_side_stream():
    case = garbage(case_ragged())
    a, b = device(case), device(case)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    c = device(case, stream=side)
    for n in a:
        assert a[n].tobytes() == b[n].tobytes() == c[n].tobytes(), n


def test_short_workspace_is_an_error_and_writes_nothing():
    import ctypes
    import kaldi_lstm_amd as k
    lib = k.load_library()
    case = garbage(generated(0, 3, 8, 12))
    S, N, stride = case["hyp"].shape
    t = {n: torch.from_numpy(case[n]).cuda() for n in ("hyp", "hyp_len", "count", "logp")}
    need = k.ctc_consensus_workspace_bytes(S, N, stride, False)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    outs = [torch.full((S * N * N,), -77, dtype=torch.int32, device="cuda") for _ in range(9)]
    totals = torch.full((10,), -77.0, dtype=torch.float64, device="cuda")

    def call(nbytes):
        p = [o.data_ptr() for o in outs]
        return lib.klstm_ctc_consensus(t["hyp"].data_ptr(), stride, t["hyp_len"].data_ptr(), t["count"].data_ptr(), t["logp"].data_ptr(), None,
                                       S, N, stride, 1.0, -1, 1, p[0], p[1], p[2], p[3], p[4], p[5], p[6], stride, p[7], totals.data_ptr(),
                                       ws.data_ptr(), ctypes.c_size_t(nbytes), None)
    assert call(need - 1) == 1 and lib.klstm_last_error().startswith(b"klstm_ctc_consensus: workspace")
    torch.cuda.synchronize()
    assert all((o == -77).all() for o in outs) and (totals == -77).all()
    assert call(need) == 0
    torch.cuda.synchronize()
    assert (outs[0][:S] >= 0).all() and totals[0] == -77 + S
