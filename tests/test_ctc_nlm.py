"""Rescoring of CTC n-best lists with an LSTM language model, host side (no GPU): the numpy twin the GPU tests are held against
(tests/ctc_nlm_ref.py) against an independent brute force (plain Python loops per entry, a tiny LSTMP written out from the equations,
math.log / math.exp in float64, sorted with a key), the LM training helper, the limits and argument errors of the knlm_* entries, and
their ABI."""
import ctypes
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from oracle.oracle import split_blob
from tests import ctc_nlm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def f32(v):
    """a Python float rounded to float32, without numpy"""
    return struct.unpack("f", struct.pack("f", v))[0] if math.isfinite(v) else v


def sigm(x):
    return 1.0 / (1.0 + np.exp(-x))


def brute_lstmp(flat, I, C, R_, xs):
    """one LstmProjectedStreams layer over the rows xs from zero state, from the equations: g, i, f, o stacked in that order, peepholes
    from c(t-1) into i and f and from c(t) into o, the cell kept within +-50, r = W_rm (o * tanh c)"""
    p = split_blob(np.asarray(flat, np.float64), I, C, R_)
    Wx, Wr, b = p["w_gifo_x"], p["w_gifo_r"], p["bias"]
    c, r, out = np.zeros(C), np.zeros(R_), []
    for x in xs:
        a = Wx @ x + Wr @ r + b
        g, i = np.tanh(a[:C]), sigm(a[C:2 * C] + p["peephole_i_c"] * c)
        f = sigm(a[2 * C:3 * C] + p["peephole_f_c"] * c)
        c = np.clip(f * c + i * g, -50.0, 50.0)
        o = sigm(a[3 * C:] + p["peephole_o_c"] * c)
        r = p["w_r_m"] @ (o * np.tanh(c))
        out.append(r)
    return out


def brute(lm, lists, logps, K, max_len, am_scale, nlm_scale, unit_bonus):
    """ONE stream: lists of tokens (any length, any tokens) with their logp -> dict(z: per entry a float, "dropped" or "forbidden",
    logp: per entry the LM's score or None, order)"""
    V = lm.W.shape[0]
    zs, lws = [], []
    for toks, lp0 in zip(lists, logps):
        if not math.isfinite(float(lp0)) or len(toks) > max_len or any(t < 0 or t >= K for t in toks):
            zs.append("dropped")
            lws.append(None)
            continue
        xs = [lm.bos] + list(toks)
        tg = list(toks) + [lm.eos]
        if lm.eos < 0:
            xs, tg = xs[:-1], tg[:-1]
        rows = []
        for x in xs:
            if lm.embed is None:
                rows.append(np.eye(V)[x])
            else:
                rows.append(np.array([f32(float(lm.embed[0][d, x]) + float(lm.embed[1][d])) for d in range(lm.embed[0].shape[0])]))
        for flat, I, C, R_ in lm.layers:
            rows = brute_lstmp(flat, I, C, R_, rows)
        total = 0.0
        for r, t in zip(rows, tg):
            a = [float(np.dot(lm.W[j].astype(np.float64), r)) + float(lm.b[j]) for j in range(V)]
            m = max(a)
            total += f32((a[t] - m) - math.log(sum(math.exp(v - m) for v in a)))
        lws.append(total)
        if not math.isfinite(total):
            zs.append("forbidden")
            continue
        zs.append(float(np.float32(am_scale)) * float(np.float32(lp0)) + float(np.float32(nlm_scale)) * total
                  + float(np.float32(unit_bonus)) * len(toks))
    order = sorted((q for q in range(len(zs)) if isinstance(zs[q], float)), key=lambda q: (-zs[q], q))
    return dict(z=zs, logp=lws, order=order)


CASES = {
    # name: (K, V, bos, eos, layers, embedding rows)
    "blank_is_bos_and_eos": (6, 6, 0, 0, 1, None),
    "no_end_term": (6, 6, 0, -1, 1, None),
    "own_class": (6, 7, 6, 6, 2, None),
    "embedding": (6, 7, 6, 6, 1, 8),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_twin_against_brute_force(case):
    K, V, bos, eos, n_lstm, D = CASES[case]
    lm = R.make_lm(K, V, bos, eos, n_lstm=n_lstm, D=D)
    kw = dict(am_scale=0.9, nlm_scale=0.7, unit_bonus=0.3)
    hyp, hyp_len, count, logp, errors = R.poisoned_lists(K=K, max_len=7, more_streams=True)
    S, N, stride = hyp.shape
    o = R.rescore(hyp, hyp_len, count, logp, K, lm, max_len=7, errors=errors, **kw)
    assert o["status"] == ["done", "done", "done", "idle", "rejected"]
    assert o["totals"][:4].tolist() == [3, 2, 2, 0]                   # one entry with a token >= K, one with NaN logp
    assert o["z64"][2, 0] == o["z64"][2, 1] and list(o["order"][2]).index(0) + 1 == list(o["order"][2]).index(1)    # equal z: the lower q first
    assert o["units"][0].tolist() == [0, 7, 0] and o["positions"][0].tolist() == [1 if eos >= 0 else 0, 7 + (eos >= 0), 0]
    worst = 0.0
    for s in range(3):
        lists = [hyp[s, q, :max(hyp_len[s, q], 0)].tolist() for q in range(count[s])]
        b = brute(lm, lists, logp[s, :count[s]], K, 7, **kw)
        assert o["order"][s, :o["live_count"][s]].tolist() == b["order"], s
        for q in range(count[s]):
            if isinstance(b["z"][q], float):
                worst = max(worst, abs(o["z64"][s, q] - b["z"][q]), abs(o["acc"][s, q] - b["logp"][q]))
            else:
                assert np.isnan(o["z64"][s, q]) and o["score"][s, q] == -np.inf and o["nlm_logp"][s, q] == -np.inf
    print(f"twin vs brute force ({case}): {worst:.3g}", flush=True)
    assert worst <= 1e-10                                                # float64 against float64; every lp rounds to the same float
    # the new 1-best's errors, the gathered list
    for s in range(3):
        for r in range(o["out_count"][s]):
            q = o["order"][s, r]
            assert o["out_hyp"][s, r, :o["out_len"][s, r]].tolist() == hyp[s, q, :hyp_len[s, q]].tolist() and o["out_errors"][s, r] == errors[s, q]
    assert o["totals"][5] == errors[:3, 0].sum() and o["totals"][6] == sum(errors[s, o["order"][s, 0]] for s in range(3))
    assert o["totals"][7] == o["positions"].sum()
    # what may not be read is not read: another poison, the same result
    hyp2, hyp_len2, count2, logp2, _ = R.poisoned_lists(K=K, max_len=7, more_streams=True, poison=-5)
    hyp_len2[hyp_len2 == -7] = 3
    logp2[np.isnan(logp2) & (np.arange(N)[None, :] >= np.clip(count2, 0, N)[:, None])] = 0.0
    o2 = R.rescore(hyp2, hyp_len2, count2, logp2, K, lm, max_len=7, errors=errors, **kw)
    for k in ("order", "live_count", "score", "nlm_logp", "units", "out_hyp", "out_len", "out_count", "out_score", "out_errors", "totals"):
        assert np.array_equal(o[k], o2[k], equal_nan=True), k


def test_float32_mode_is_close_to_float64():
    lm = R.make_lm(6, 6, 0, 0, n_lstm=2)
    hyp, hyp_len, count, logp, _ = R.poisoned_lists()
    a64, p64, x64 = R.score_entries(hyp, hyp_len, count, logp, 6, lm, 7)
    a32, p32, x32 = R.score_entries(hyp, hyp_len, count, logp, 6, lm, 7, dtype=np.float32)
    assert np.array_equal(p64, p32) and 0 < np.abs(x64 - x32).max() < 1e-4       # before lp is rounded to float the two nets differ ...
    assert np.abs(a64 - a32).max() < 1e-4 and np.abs(a64 - x64).max() < 8 * 2.0 ** -24 * 4    # ... and the rounding costs half an ulp of lp (< 4) a position


def test_rank_forbids_what_is_not_finite_and_ranks_ties_by_q():
    hyp, hyp_len, count, logp, errors = R.poisoned_lists()
    acc = np.array([[-1.0, -np.inf, 5.0], [3.0, np.nan, 9.0], [-2.0, -2.0, -2.5]])
    o = R.rank(hyp, hyp_len, count, logp, 6, acc, True, errors=errors, max_len=7)
    assert o["order"].tolist() == [[0, -1, -1], [-1, -1, -1], [0, 1, 2]] and o["status"] == ["done", "idle", "done"]
    assert o["totals"].tolist() == [2, 1, 2, 2, 0, errors[0, 0] + errors[2, 0], errors[0, 0] + errors[2, 0], 1 + 8 + 4 + 6 + 6 + 7]
    o = R.rank(hyp, hyp_len, count, logp, 6, acc, False, unit_bonus=10.0, max_len=7, out_n=1)
    assert o["order"][2].tolist() == [2, 0, 1] and o["totals"][4] == 1 and o["out_count"].tolist() == [1, 0, 1]
    assert o["out_errors"].tolist() == [[-1]] * 3 and o["totals"][7] == 0 + 7 + 3 + 5 + 5 + 6


def test_pack_rows_of_the_twin():
    hyp, hyp_len, count, logp, _ = R.poisoned_lists()
    lm = R.make_lm(6, 7, 6, 6)
    x = R.pack_rows(hyp, hyp_len, count, logp, 6, lm, first_entry=0, E=4, T=3, t0=0, max_len=7)
    assert x.shape == (12, 7) and x[0].tolist() == [0, 0, 0, 0, 0, 0, 1] and x[4].sum() == 0        # the empty entry: bos, then nothing
    assert x[1, 6] == 1 and x[4 + 1, hyp[0, 1, 0]] == 1 and x[2].sum() == 0 and x[3].sum() == 0    # a token >= K, NaN logp: zero rows
    x = R.pack_rows(hyp, hyp_len, count, logp, 6, lm, first_entry=0, E=4, T=3, t0=6, max_len=7)
    assert x[1, hyp[0, 1, 5]] == 1 and x[4 + 1, hyp[0, 1, 6]] == 1 and x[8 + 1].sum() == 0           # positions 6, 7 (the end term's input), 8
    x = R.pack_rows(hyp, hyp_len, count, logp, 6, lm, first_entry=8, E=4, T=3, t0=0, max_len=7)
    assert x[0, 6] == 1 and x[1:4].sum() == 0                                                         # entry 8 alone in its group


def test_lm_training_utterances():
    import kaldi_lstm_amd as k
    utts = k.lm_training_utterances([[3, 1, 2], [], [5]], 7, 6, 0)
    assert [u[0].shape for u in utts] == [(4, 7), (1, 7), (2, 7)] and all(u[0].dtype == np.float32 and u[1].dtype == np.int32 for u in utts)
    assert utts[0][0].argmax(1).tolist() == [6, 3, 1, 2] and utts[0][1].tolist() == [3, 1, 2, 0] and (utts[0][0].sum(1) == 1).all()
    assert utts[1][0].argmax(1).tolist() == [6] and utts[1][1].tolist() == [0]
    utts = k.lm_training_utterances([[3, 1, 2], []], 7, 6, -1)
    assert len(utts) == 1 and utts[0][0].argmax(1).tolist() == [6, 3, 1] and utts[0][1].tolist() == [3, 1, 2]
    with pytest.raises(ValueError):
        k.lm_training_utterances([[7]], 7, 6, 0)


def test_refused_shapes_and_arguments_without_a_gpu():
    import kaldi_lstm_amd as k
    lib = k.load_library()
    q = lib.knlm_workspace_bytes
    for a in [(1, 1), (32, 20), (16, 1000)]:
        assert q(*a) > 0, a
    for a in [(0, 20), (33, 20), (16, 0), (32, (1 << 19) + 1)]:
        assert q(*a) == 0 and lib.klstm_last_error().startswith(b"knlm_workspace_bytes:"), a
    with pytest.raises(k.KlstmError) as ei:
        k.knlm_workspace_bytes(33, 20)
    assert ei.value.status == 2
    p = ctypes.c_void_p(256)                            # never dereferenced: refused before any pointer is followed
    big = ctypes.c_size_t(1 << 30)

    def pack(S=3, N=3, L=7, K=6, V=7, bos=6, eos=6, first=0, E=4, T=3, t0=0, hyp=p, out=p, emb=None, bias=None, D=0, stride=9, ostride=8):
        return lib.knlm_pack(hyp, stride, p, p, p, S, N, L, K, V, bos, eos, first, E, T, t0, emb, bias, D, out, ostride, None)

    def rows(S=3, N=3, L=7, K=6, V=7, eos=6, first=0, E=4, T=3, t0=0, a=p, acc=p, ws=p, wsb=big, stride=9, astride=7):
        return lib.knlm_score_rows(a, astride, p, stride, p, p, p, S, N, L, K, V, eos, first, E, T, t0, acc, None, ws, wsb, None)

    def rank(S=3, N=3, L=7, K=6, acc=p, am=1.0, ns=1.0, ub=0.0, out_n=0, order=p, stride=9, ostride=9, out_hyp=p):
        return lib.knlm_rank(p, stride, p, p, p, None, S, N, L, K, acc, am, ns, ub, 1, order, p, p, None, None, out_n, out_hyp, ostride, p, p, p, None,
                             None, None)
    shape = [dict(S=0), dict(S=33), dict(N=0), dict(N=65), dict(L=-1), dict(L=1024), dict(K=1)]
    for fn, name, more in ((pack, b"knlm_pack:", [dict(V=5), dict(V=32769), dict(E=0), dict(E=33), dict(T=0), dict(emb=p, bias=p, D=0), dict(emb=p, bias=p, D=32769)]),
                           (rows, b"knlm_score_rows:", [dict(V=5), dict(V=32769), dict(E=0), dict(E=33), dict(T=0)]),
                           (rank, b"knlm_rank:", [dict(K=32769), dict(out_n=4), dict(out_n=-1)])):
        for kw in shape + more:
            assert fn(**kw) == 2 and lib.klstm_last_error().startswith(name), (name, kw)
    for kw in (dict(hyp=None), dict(out=None), dict(emb=p, bias=None, D=8), dict(bos=-1), dict(bos=7), dict(eos=7), dict(first=-1), dict(first=9),
               dict(t0=-1), dict(stride=0), dict(ostride=6), dict(emb=p, bias=p, D=8, ostride=7)):
        assert pack(**kw) == 1 and lib.klstm_last_error().startswith(b"knlm_pack:"), kw
    for kw in (dict(a=None), dict(acc=None), dict(ws=None), dict(eos=7), dict(first=-1), dict(first=9), dict(t0=-1), dict(stride=0), dict(astride=6),
               dict(ws=ctypes.c_void_p(264)), dict(wsb=ctypes.c_size_t(lib.knlm_workspace_bytes(4, 3) - 1))):
        assert rows(**kw) == 1 and lib.klstm_last_error().startswith(b"knlm_score_rows:"), kw
    for kw in (dict(acc=None), dict(order=None), dict(am=float("nan")), dict(ns=float("inf")), dict(ub=float("-inf")), dict(out_n=2, out_hyp=None),
               dict(stride=0), dict(out_n=2, ostride=6)):
        assert rank(**kw) == 1 and lib.klstm_last_error().startswith(b"knlm_rank:"), kw
    for name in ("CtcNeuralLm", "CtcNeuralRescoreResult", "knlm_pack", "knlm_score_rows", "knlm_rank", "knlm_workspace_bytes", "lm_training_utterances"):
        assert hasattr(k, name)
    with pytest.raises(ValueError):                     # the topology is checked before a device is touched
        k.CtcNeuralLm([(np.zeros(10, np.float32), 5, 16, 8)], np.zeros((6, 8), np.float32), np.zeros(6, np.float32))


def declared_names():
    txt = open(os.path.join(ROOT, "include", "klstm_nlm.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(knlm_[a-z_0-9]+)\s*\(", txt)))


def test_abi_of_the_knlm_family():
    """every knlm_* name include/klstm_nlm.h declares is exported, and the names the library defines are those of
    tests/golden/knlm_abi_names.txt; include/klstm.h declares none of them"""
    import kaldi_lstm_amd as k
    lib = k.load_library()
    names = declared_names()
    assert len(names) == 4
    for n in names:
        assert hasattr(lib, n), f"libklstm.so does not export {n}"
    out = subprocess.run(["nm", "-D", "--defined-only", k.lib_path()], capture_output=True, text=True, check=True).stdout
    have = sorted({ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("knlm_")})
    want = open(os.path.join(ROOT, "tests", "golden", "knlm_abi_names.txt")).read().split()
    assert want == sorted(want) and have == want == names, f"lost {sorted(set(want) - set(have))}, added {sorted(set(have) - set(want))}"
    klstm_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "klstm.h")).read(), flags=re.S)
    assert "knlm_" not in klstm_h


def test_cpp_driver_builds():
    from tests import cpp_driver
    r = cpp_driver.run("ctc_nlm_test", ok=False, timeout=300, headers=cpp_driver.HEADERS + ("klstm_nlm.h",))
    assert r.returncode == 2 and "usage: ctc_nlm_test" in r.stderr


@pytest.mark.parametrize("eos", [0, -1])
def test_cpp_lm_training_utterances_mirror_the_python_ones(eos):
    """LmTrainingUtterances (include/klstm_nnet.hpp) through the driver, host only: one-hot rows [bos, y...] and targets [y..., eos], an
    empty sequence skipped without an end term -- the utterances kaldi_lstm_amd.lm_training_utterances makes"""
    import kaldi_lstm_amd as k
    from tests import cpp_driver
    r = cpp_driver.run("ctc_nlm_test", "utterances", 7, 6, eos, timeout=300, headers=cpp_driver.HEADERS + ("klstm_nlm.h",))
    lines = r.stdout.strip().split("\n")
    want = k.lm_training_utterances([[3, 1, 2], [], [5]], 7, 6, eos)
    assert lines[0] == "OK %d" % len(want) and len(lines) == 1 + len(want) and len(want) == (3 if eos >= 0 else 2)
    for ln, (f, t) in zip(lines[1:], want):
        shape, hot, tgt, sizes = (part.split() for part in ln.split(":"))
        assert [int(v) for v in shape] == [f.shape[0], 7] and [int(v) for v in hot] == f.argmax(1).tolist() and (f.sum(1) == 1).all()
        assert [int(v) for v in tgt] == t.tolist() and [int(v) for v in sizes] == [f.size, 0]
