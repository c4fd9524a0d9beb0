"""Second-pass rescoring of n-best lists, host side (no GPU): the numpy twin the GPU tests are held against (tests/ctc_rescore_ref.py
rescore) against an independent brute force (dense expansion of the model, math.fsum of math.log, Python sorted), the word table and the
host helpers of lm.py, the limits and argument errors of the library's entry, and the conditions of the GPU cases."""
import ctypes
import os

import numpy as np
import pytest

from tests import cpp_driver
from tests import ctc_consensus_ref as C
from tests import ctc_rescore_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_ctc_rescore_driver():
    return cpp_driver.build("ctc_rescore_test")


def run_driver(*args, ok=True):
    return cpp_driver.run("ctc_rescore_test", *args, ok=ok, timeout=300)


@pytest.fixture(scope="module")
def models():
    corpus, bigram, order4 = R.token_models()
    return dict(corpus=corpus, bigram=bigram, order4=order4)


@pytest.fixture(scope="module")
def wordset():
    return R.word_setup()


def rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


@pytest.mark.parametrize("mode", ["add", "sub+add", "add_nofinal", "sub"])
def test_twin_against_brute_force_tokens(models, mode):
    hyp, hyp_len, count, logp = R.lists_from_corpus(1, models["corpus"], 4, 8, 12)
    add = None if mode == "sub" else models["order4"]._replace(final=None) if mode == "add_nofinal" else models["order4"]
    sub = models["bigram"] if "sub" in mode else None
    kw = dict(am_scale=0.9, add_scale=0.7, unit_bonus=0.3)
    o = R.rescore(hyp, hyp_len, count, logp, 12, sub=sub, add=add, **kw)
    worst = 0.0
    for s in range(4):
        lists = [hyp[s, q, :hyp_len[s, q]].tolist() for q in range(8)]
        b = R.brute(lists, logp[s], sub=sub, add=add, **kw)
        assert o["order"][s].tolist() == b["order"]
        for q in range(8):
            worst = max(worst, rel(o["z64"][s, q], b["z"][q]))
    print(f"twin vs brute force: {worst:.3g}", flush=True)
    assert worst <= 1e-12


def test_twin_logw_against_brute_force_in_double(models):
    """logw itself, in double, to 1e-12 relative"""
    worst = 0.0
    for seq in models["corpus"][:20]:
        for m in (models["bigram"], models["order4"]):
            f, _, _, lw = R.walk(m, seq)
            b = R.brute([seq], [0.0], add=m)
            assert not f
            worst = max(worst, rel(lw, b["add_logw"][0]))
    assert worst <= 1e-12


def test_twin_against_brute_force_words(wordset):
    ws = wordset
    hyp, hyp_len, count, logp = R.word_lists(ws)
    vocab = {tuple(w): i for i, w in enumerate(ws["vocab"])}
    for unk in (ws["unk"], -1):
        o = R.rescore(hyp, hyp_len, count, logp, ws["K"], add=ws["model"], words=R.Words(*ws["table"], unk, ws["sep"]), add_reserved=ws["reserved"],
                      add_scale=0.8, unit_bonus=0.5)
        for s in range(hyp.shape[0]):
            lists = [hyp[s, q, :hyp_len[s, q]].tolist() for q in range(hyp.shape[1])]
            b = R.brute(lists, logp[s], add=ws["model"], vocab=vocab, unk_id=unk, separator=ws["sep"], add_scale=0.8, unit_bonus=0.5)
            assert o["order"][s, :o["live_count"][s]].tolist() == b["order"]
            for q in b["order"]:
                assert rel(o["z64"][s, q], b["z"][q]) <= 1e-12
            assert [q for q in range(len(lists)) if b["z"][q] is None] == [q for q in range(len(lists)) if np.isnan(o["z64"][s, q])]
        assert o["oov"].sum() >= 1                                   # a condition of the GPU case


def test_word_table_and_sequences():
    import kaldi_lstm_amd as k
    words = [[3, 1], [2], [1, 3], [5, 5, 5]]
    keys, ids = k.word_table(words, 0)
    assert keys.dtype == np.uint64 and ids.dtype == np.int32 and (np.diff(keys.astype(object)) > 0).all()
    assert sorted(int(x) for x in keys) == sorted(C.word_key(w) for w in words)
    assert all(int(keys[list(ids).index(i)]) == C.word_key(w) == k.word_key(w) for i, w in enumerate(words))
    assert C.units_of([0, 3, 1, 0, 0, 2], 0) == [k.word_key([3, 1]), k.word_key([2])]
    with pytest.raises(ValueError):
        k.word_table(words + [[2]], 0)
    keys2, ids2 = k.word_table(words, 0, ids=[7, 8, 9, 10])
    assert np.array_equal(keys2, keys) and sorted(ids2.tolist()) == [7, 8, 9, 10]
    seqs = k.word_sequences([[3, 1, 0, 2], [0, 2, 0, 0, 4, 0], [], [1, 3]], (keys, ids), 0, 9)
    assert seqs == [[0, 1], [1, 9], [], [2]]
    assert k.word_sequences([[3, 1, 0, 2], [4]], (keys, ids), 0, -1) == [[0, 1]]
    t = R.Words(keys, ids, 9, 0)
    assert t.lookup(k.word_key([2]), 4, 3) == (1, False) and t.lookup(k.word_key([4]), 4, 3) == (9, True)
    assert t.lookup(k.word_key([5, 5, 5]), 4, 3) == (9, True) and t.lookup(k.word_key([5, 5, 5]), 3, 2) == (9, True)


def test_hash_constants_of_python_and_twins_are_the_macros_of_klstm_h():
    """lm.py and tests/nbest_ref.py cannot see include/klstm.h: their literals are held against its two macros, read as text"""
    import re

    import kaldi_lstm_amd.lm as LM
    from tests import nbest_ref
    text = open(os.path.join(ROOT, "include", "klstm.h")).read()
    macro = {n: int(v, 16) for n, v in re.findall(r"^#define (KLSTM_CTC_HASH_\w+)\s+(0x[0-9A-Fa-f]+)ull\b", text, re.M)}
    assert sorted(macro) == ["KLSTM_CTC_HASH_MUL", "KLSTM_CTC_HASH_START"]
    assert (LM._WORD_H0, LM._WORD_HMUL) == (macro["KLSTM_CTC_HASH_START"], macro["KLSTM_CTC_HASH_MUL"]) == (nbest_ref.H0, nbest_ref.HMUL)
    assert LM.split_words([0, 3, 1, 0, 0, 2, 0], 0) == nbest_ref.split_words([0, 3, 1, 0, 0, 2, 0], 0) == [[3, 1], [2]]
    assert LM.split_words([0, 0], 0) == LM.split_words([], 0) == []


def test_dense_lm_to_sparse():
    import kaldi_lstm_amd as k
    K, blank = 6, 0
    seqs = [[1, 2, 3], [2, 2, 5], [4, 1], [3]]
    dense = k.ngram_label_lm(seqs, K, blank, order=2)
    sp = k.dense_lm_to_sparse(*dense, blank=blank)
    model, status = k.sparse_lm_validate(sp, blank)
    assert status[:6] == [0] * 6
    nxt, wt, fin = k.sparse_lm_to_dense(sp)
    keep = dense[1] > 0
    assert np.array_equal(wt, dense[1]) and np.array_equal(nxt[keep], dense[0][keep]) and (nxt[~keep] == -1).all()
    lex = k.lexicon_label_lm([[2, 3], [4]], K, blank, 1)
    sp = k.dense_lm_to_sparse(*lex, blank=blank)
    assert R.walk(sp, [2, 3, 1, 4])[0] is False and R.walk(sp, [2, 4])[0] is True and R.walk(sp, [2])[0] is True


def test_walk_rules_on_hand_written_cases():
    m = R.forbidding_model()
    assert [R.walk(m, u)[0] for u in ([1, 1], [2], [1, 2], [3], [1], [])] == [False, True, True, True, True, False]
    f, mant, e, lw = R.walk(m, [1, 1])
    assert (mant, e) == (0.5, -2) and lw == np.log(0.5) - 2 * R.LN2
    assert R.walk(m, [])[1:3] == (0.5, 0)
    assert R.walk(m._replace(final=None), [])[1:] == (1.0, 0, 0.0)
    o = R.rescore(*R.pack([[[1, 1], [1, 1], [2]]]), np.array([[-1.0, -1.0, 0.0]], np.float32), 4, add=m)
    assert o["order"][0].tolist() == [0, 1, -1] and o["totals"].tolist() == [1, 0, 0, 1, 0, 0, 0, 0]
    o = R.rescore(*R.pack([[[1, 1], [1, 1, 1, 1]]]), np.array([[-1.0, -1.0]], np.float32), 4, add=m, unit_bonus=3.0)
    assert o["order"][0].tolist() == [1, 0] and o["totals"][4] == 1


def test_conditions_of_the_gpu_cases(models, wordset):
    """held here first, from the twin: back-off depths 0 to 3 in the order-4 case; a changed 1-best; direct rows and bisected states"""
    import kaldi_lstm_amd as k
    hyp, hyp_len, count, logp = R.lists_from_corpus(1, models["corpus"], 4, 8, 12)
    depths = []
    o = R.rescore(hyp, hyp_len, count, logp, 12, add=models["order4"], add_scale=0.7, unit_bonus=0.3, depths=depths)
    assert {0, 1, 2, 3} <= set(depths)
    assert (o["order"][:, 0] != 0).any() and o["totals"][4] >= 1
    assert R.min_gap(o) >= 1e-9
    _, st = k.sparse_lm_validate(models["bigram"], 0)
    assert st[6] == len(models["bigram"].backoff)                    # every state of the bigram is a direct row on the device
    _, st = k.sparse_lm_validate(models["order4"], 0)
    assert 0 < st[6] < len(models["order4"].backoff)                 # the order-4 model has bisected states
    assert wordset["V"] == 32 and all(1 <= len(w) <= 4 for w in wordset["vocab"]) and len(wordset["vocab"]) == 30


def test_refused_shapes_and_arguments_without_a_gpu():
    import kaldi_lstm_amd as k
    lib = k.load_library()
    q = lib.klstm_ctc_rescore_workspace_bytes
    for a in [(1, 1, 0, 0), (32, 64, 1023, 1), (8, 64, 255, 0)]:
        assert q(*a) > 0, a
    for a in [(8, 65, 60, 0), (8, 8, 1024, 0), (0, 8, 60, 0), (33, 8, 60, 0), (8, 0, 60, 1), (8, 8, -1, 0)]:
        assert q(*a) == 0 and b"klstm_ctc_rescore_workspace_bytes" in lib.klstm_last_error(), a
    with pytest.raises(k.KlstmError) as ei:
        k.ctc_rescore_workspace_bytes(8, 65, 60)
    assert ei.value.status == 2
    p = ctypes.c_void_p(256)                            # never dereferenced: refused before any pointer is followed
    z = ctypes.c_size_t(1 << 20)

    def call(S=4, N=8, L=60, K=12, sub=p, add=p, add_classes=12, W=0, unk=-1, sep=-1, reserved=-1, am=1.0, out_n=0, hyp=p, ws=p,
             wsb=ctypes.c_size_t(1 << 30), keys=None, stride=60, out_stride=60):
        return lib.klstm_ctc_nbest_rescore(hyp, stride, p, p, p, None, S, N, L, K, sub, z, 5, None, add, z, 5, add_classes, None, keys, keys, W, unk,
                                           sep, reserved, am, 1.0, 0.0, p, p, p, None, None, None, None, out_n, p, out_stride, p, p, p, None, None,
                                           ws, wsb, None)
    for kw in (dict(N=65), dict(L=1024), dict(S=0), dict(S=33), dict(W=(1 << 24) + 1), dict(W=-1), dict(out_n=9), dict(out_n=-1), dict(K=1),
               dict(K=32769)):
        assert call(**kw) == 2 and lib.klstm_last_error().startswith(b"klstm_ctc_nbest_rescore:"), kw
    for kw in (dict(hyp=None), dict(ws=None), dict(sub=None, add=None), dict(am=float("nan")), dict(am=float("inf")), dict(sub=p, add=None, W=3, keys=p),
               dict(W=3), dict(W=3, keys=p, sep=12, reserved=0, add_classes=5), dict(W=3, keys=p, sep=0, reserved=5, add_classes=5),
               dict(W=3, keys=p, sep=0, reserved=4, unk=4, add_classes=5), dict(W=3, keys=p, sep=0, reserved=4, unk=5, add_classes=5),
               dict(add_classes=11), dict(stride=0), dict(out_n=2, out_stride=59),
               dict()):                                  # the last: no model was built at address 256
        assert call(**kw) == 1 and lib.klstm_last_error().startswith(b"klstm_ctc_nbest_rescore:"), kw
    assert b"no sparse language model was built" in lib.klstm_last_error()
    for name in ("ctc_nbest_rescore", "CtcWordTable", "ctc_rescore_workspace_bytes", "word_table", "word_sequences", "dense_lm_to_sparse"):
        assert hasattr(k, name)


def test_cpp_driver_builds():
    r = run_driver(ok=False)
    assert r.returncode == 2 and "usage: ctc_rescore_test" in r.stderr
