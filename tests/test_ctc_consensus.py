"""MBR decoding and unit confidences over n-best lists, host side (no GPU): the numpy twin the GPU tests are held against
(tests/ctc_consensus_ref.py consensus) against an independent brute force (full tables in Python ints, math.fsum), the alignment rule
and the word tokenisation on hand-written cases, and the limits of the library's entry."""
import ctypes
import itertools

import numpy as np
import pytest

from tests import cpp_driver
from tests import ctc_consensus_ref as C
from tests import nbest_ref



def build_ctc_consensus_driver():
    return cpp_driver.build("ctc_consensus_test")


def run_driver(*args, ok=True):
    return cpp_driver.run("ctc_consensus_test", *args, ok=ok, timeout=300)


def pack(lists, stride=None):
    """nbest_ref.pack with garbage in what the device may not read"""
    return nbest_ref.pack(lists, stride, fill=10 ** 6, len_fill=-7)


@pytest.mark.parametrize("seed,N,L,sep", [(0, 2, 1, -1), (1, 8, 12, -1), (2, 16, 30, -1), (3, 8, 40, 3), (4, 5, 0, -1)])
@pytest.mark.parametrize("pivot_mode", [0, 1])
def test_twin_against_brute_force(seed, N, L, sep, pivot_mode):
    S = 3
    hyp, hyp_len, count, logp = C.make_lists(seed, S, N, L, K=6 if sep >= 0 else 9, spread=3.0)
    scale = [0.5, 1.0, 3.0][seed % 3]
    o = C.consensus(hyp, hyp_len, count, logp, scale=scale, separator=sep, pivot_mode=pivot_mode)
    worst = 0.0
    for s in range(S):
        lists = [hyp[s, q, :hyp_len[s, q]].tolist() for q in range(N)]
        b = C.brute(lists, logp[s], scale, sep, pivot_mode)
        D = o["dist"][s]
        assert np.array_equal(D, np.array(b["dist"]))
        assert np.array_equal(D, D.T) and not np.diag(D).any()
        for q, r, t in itertools.product(range(N), repeat=3):
            assert D[q, r] <= D[q, t] + D[t, r]
        assert (o["map"][s], o["mbr"][s], o["pick"][s]) == (b["map"], b["mbr"], b["pick"])
        n = len(b["conf"])
        assert o["conf_len"][s] == n == o["unit_len"][s, b["pick"]]
        worst = max(worst, np.abs(o["risk64"][s] - b["risk"]).max(), np.abs(o["post64"][s] - b["post"]).max(),
                    np.abs(o["conf64"][s, :n] - b["conf"]).max() if n else 0.0)
        assert (o["conf64"][s, :n] >= o["post64"][s, b["pick"]]).all()           # the pivot is matched against itself
        assert (o["conf64"][s, :n] <= 1 + 1e-15).all()
    print(f"twin vs brute force: {worst:.3g}", flush=True)
    assert worst <= 1e-12


def test_one_live_entry_has_confidence_one():
    hyp, hyp_len, count = pack([[[1, 2, 3], [4]], [[5, 5]]])
    logp = np.array([[-1.0, -np.inf], [-2.0, 0.0]], np.float32)
    o = C.consensus(hyp, hyp_len, count, logp)
    assert o["pick"].tolist() == [0, 0] and (o["conf64"][0, :3] == 1).all() and (o["conf64"][1, :2] == 1).all()
    assert o["post"][0].tolist() == [1, 0] and o["risk"][0].tolist() == [0, -1] and o["dist"][0].tolist() == [[0, -1], [-1, -1]]
    assert o["totals"].tolist() == [2, 0, 0, 0, 0, 5, 5, 1, 0, 0]


def test_alignment_rule_on_hand_written_cases():
    m = C.matched
    assert m([1, 1], [1]) == [False, True]             # the diagonal first: the LAST 1 is the matched one
    assert m([1], [1, 1]) == [True]                    # (1, 2): diagonal with the second 1
    assert m([1, 2, 3], [1, 3]) == [True, False, True]
    assert m([1, 2, 3], [4, 2, 5]) == [False, True, False]
    assert m([1, 2], []) == [False, False] and m([], [1]) == []
    assert m([1, 2, 1], [2, 1]) == [False, True, True]
    assert m([2, 1], [1, 2, 1]) == [True, True]
    assert m([1, 2], [2, 1]) == [False, False]         # two substitutions by the diagonal, not delete + match + insert


def test_word_mode_tokenisation():
    sep = 0
    u = C.units_of
    assert u([0, 0, 0], sep) == [] and u([], sep) == []
    one = u([1, 2], sep)
    assert len(one) == 1 and one[0] == C.word_key([1, 2]) != C.word_key([2, 1])
    assert u([0, 1, 2], sep) == one and u([1, 2, 0], sep) == one and u([0, 0, 1, 2, 0, 0], sep) == one
    assert u([1, 0, 0, 2], sep) == [C.word_key([1]), C.word_key([2])] == u([0, 1, 0, 2, 0], sep)
    assert u([1, 2], -1) == [1, 2]
    # the hash of klstm_ctc_dev.h on a value worked by hand: ((H0 ^ 2) * HMUL mod 2^64) folded once
    x = ((C.H0 ^ 2) * C.HMUL) % 2 ** 64
    assert C.word_key([1]) == x ^ (x >> 29)
    hyp, hyp_len, count = pack([[[0, 1, 2, 0, 0, 3], [1, 2, 0, 3, 0], [0, 0], [1, 0, 2, 0, 3]]])
    o = C.consensus(hyp, hyp_len, count, np.array([[-1.0, -1.5, -2.0, -2.5]], np.float32), separator=sep)
    assert o["unit_len"][0].tolist() == [2, 2, 0, 3]
    assert o["dist"][0].tolist() == [[0, 0, 2, 2], [0, 0, 2, 2], [2, 2, 0, 3], [2, 2, 3, 0]]
    t = C.consensus(hyp, hyp_len, count, np.array([[-1.0, -1.5, -2.0, -2.5]], np.float32))
    assert t["unit_len"][0].tolist() == [6, 5, 2, 5] and t["dist"][0, 0, 1] == 3


def test_statuses_and_dropped_entries():
    hyp, hyp_len, count = pack([[[1, 2], [1], [3], [4], [5]], [[1]], [], [[1, 2]]], stride=4)
    hyp_len[0, 2] = 5                                   # above the stride
    hyp[0, 3, 0] = -1                                   # a negative token
    count[3] = 6                                        # outside [0, N]
    logp = np.array([[-1, -2, -1, -1, np.nan], [np.inf, 0, 0, 0, 0], [0] * 5, [0] * 5], np.float32)
    o = C.consensus(hyp, hyp_len, count, logp)
    assert o["pick"].tolist() == [0, -1, -1, -1]
    assert (o["risk"][0] >= 0).tolist() == [True, True, False, False, False]
    assert o["totals"][[0, 1, 7]].tolist() == [1, 3, 4]
    assert C.consensus(hyp, hyp_len, count, logp, max_len=1)["pick"].tolist() == [1, -1, -1, -1]


def test_refused_shapes_without_a_gpu():
    import kaldi_lstm_amd as k
    lib = k.load_library()
    q = lib.klstm_ctc_consensus_workspace_bytes
    for a in [(1, 1, 0, 0), (32, 64, 1023, 1), (8, 64, 255, 0)]:
        assert q(*a) > 0, a
    for a in [(8, 65, 60, 0), (8, 8, 1024, 0), (0, 8, 60, 0), (33, 8, 60, 0), (8, 0, 60, 1), (8, 8, -1, 0)]:
        assert q(*a) == 0 and b"klstm_ctc_consensus_workspace_bytes" in lib.klstm_last_error(), a
    assert q(8, 64, 60, 1) > q(8, 64, 60, 0) and q(1, 3, 1023, 0) > q(1, 3, 255, 0) + 3 * 1023 * 256 - 4096
    assert q(8, 64, 255, 0) < 1 << 20                  # up to 255 units every table of back-pointers is in LDS
    with pytest.raises(k.KlstmError) as ei:
        k.ctc_consensus_workspace_bytes(8, 65, 60)
    assert ei.value.status == 2
    p = ctypes.c_void_p(256)                            # never dereferenced: the shape is refused before any pointer is looked at
    for S, N, L in [(8, 65, 60), (8, 8, 1024), (0, 8, 60)]:
        st = lib.klstm_ctc_consensus(p, 60, p, p, p, None, S, N, L, 1.0, -1, 1, p, p, p, p, p, p, p, 60, None, None, p, ctypes.c_size_t(1 << 30), None)
        assert st == 2 and lib.klstm_last_error().startswith(b"klstm_ctc_consensus:"), (S, N, L)
    for name in ("ctc_nbest_consensus", "consensus_to_lists", "CtcConsensusResult", "ctc_consensus_workspace_bytes"):
        assert hasattr(k, name)


def test_cpp_driver_builds():
    r = run_driver(ok=False)
    assert r.returncode == 2 and "usage: ctc_consensus_test" in r.stderr
