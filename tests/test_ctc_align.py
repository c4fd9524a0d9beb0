"""CTC forced alignment, host side (no GPU): the library and the package carry the feature; the numpy twin that DEFINES what
klstm_ctc_align computes (tests/ctc_align_ref.py) against an enumeration of all paths and against the structural properties of an
alignment; the tie rule; the selection of the inputs that tests/test_ctc_align_gpu.py compares exactly; the host-side answers of the
C-ABI; and AlignCtcWholeUtterances' utterance order plus SetTargetsFromAlignment (include/klstm_nnet.hpp) through
tests/cpp/ctc_align_test."""

import numpy as np
import pytest

from tests import cpp_driver
from tests import ctc_align_ref as A
from tests import ctc_ref as R
from tests.test_ctc import plain_utts



def build_ctc_align_driver():
    return cpp_driver.build("ctc_align_test")


def run_driver(*args, ok=True):
    return cpp_driver.run("ctc_align_test", *args, ok=ok)


def validate_stream(r, n, labels, blank):
    A.validate(r["frame_class"][:n], r["frame_pos"][:n], r["token_begin"], r["token_end"], labels, blank)
    assert (r["frame_class"][n:] == -1).all() and (r["frame_pos"][n:] == -1).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the feature exists (fails on a tree without it)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_library_and_package_carry_the_aligner():
    import kaldi_lstm_amd as k
    lib = k.load_library()
    assert hasattr(lib, "klstm_ctc_align") and hasattr(lib, "klstm_ctc_align_workspace_bytes")
    assert callable(k.ctc_align) and callable(k.alignments_to_lists) and callable(k.ctc_align_workspace_bytes)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the twin against the enumeration of all paths, and its path against the definition of an alignment
# ---------------------------------------------------------------------------------------------------------------------------------
def test_twin_equals_brute_force_on_tiny_cases():
    rng = np.random.RandomState(0)
    n_cases = n_infeasible = n_repeat = 0
    for T in range(1, 7):
        for lab in ([], [1], [2], [1, 2], [2, 1], [1, 1], [2, 2]):
            for blank in (0,):
                y = rng.dirichlet(np.ones(3), size=T).astype(np.float32)
                want = A.best_brute_force(y, lab, blank)
                tw = A.align_twin(y[:, None, :], [T], [lab], blank)[0]
                n_cases += 1
                n_repeat += len(lab) == 2 and lab[0] == lab[1]
                if want is None:
                    assert tw["status"] == A.REJECTED and tw["best"] is None, (T, lab)
                    n_infeasible += 1
                    continue
                assert tw["status"] == A.ALIGNED and abs(tw["best"] - want) <= 1e-12, (T, lab, tw["best"], want)
                validate_stream(tw, T, lab, blank)
                assert abs(A.path_score64(y, tw["frame_class"][:T]) - want) <= 1e-12
    assert n_cases >= 30 and n_infeasible >= 4 and n_repeat >= 8
    # another blank, and a zero / NaN posterior on the way (counts as FLT_MIN)
    for seed, blank in ((1, 1), (2, 2)):
        y = np.random.RandomState(seed).dirichlet(np.ones(3), size=5).astype(np.float32)
        y[2, 0] = 0.0
        y[3, 1] = np.nan
        lab = [c for c in (0, 1, 2) if c != blank]
        tw = A.align_twin(y[:, None, :], [5], [lab], blank)[0]
        assert abs(tw["best"] - A.best_brute_force(y, lab, blank)) <= 1e-12
        validate_stream(tw, 5, lab, blank)


def test_twin_statuses():
    y, _ = R.make_case(2, 30, 8, 3.0, [30] * 7, [0] * 7)
    y = y.numpy()
    lens = [30, 0, 31, -1, 30, 30, 3]
    labels = [[1, 2, 3], [1], [1], [1], [1, 8, 2], [1, 0], [4, 4]]
    tw = A.align_twin(y, lens, labels, 0)
    assert [r["status"] for r in tw] == [1, 0, 2, 2, 2, 2, 1]               # stream 6: 3 frames for two equal labels, exactly feasible
    assert tw[6]["frame_class"][:3].tolist() == [4, 0, 4]
    for r in tw[1:6]:
        assert (r["frame_class"] == -1).all() and (r["token_begin"] == -1).all() and r["best"] is None
    assert A.align_twin(y[:, :1], [30], [[1] * 5], 0, max_labels=4)[0]["status"] == A.REJECTED
    assert A.align_twin(y[:, :1], [2], [[4, 4]], 0)[0]["status"] == A.REJECTED


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. ties on uniform posteriors: stay, then advance, then skip; at the end the blank
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_tie_rule_on_uniform_posteriors(dtype):
    y = np.full((20, 1, 64), 1.0 / 64, np.float32)
    b = 0

    def path(labels, n=20, blank=0):
        return A.align_twin(y[:n], [n], [labels], blank, dtype=dtype)[0]["frame_class"][:n].tolist()
    assert path([5, 5, 9]) == [5, b, 5, 9] + [b] * 16                        # the labels crammed to the front, blanks behind
    assert path([]) == [b] * 20
    assert path([7]) == [7] + [b] * 19
    assert path([1, 2, 3]) == [1, 2, 3] + [b] * 17                            # skips where the labels differ
    assert path([1, 1, 1, 1], n=7) == [1, b, 1, b, 1, b, 1]                   # exactly feasible: one path
    assert path([4, 4], n=4) == [4, b, 4, b]
    assert path([3, 3], n=20, blank=63) == [3, 63, 3] + [63] * 17
    r = A.align_twin(y, [20], [[5, 5, 9]], 0, dtype=dtype)[0]
    assert r["token_begin"].tolist() == [0, 2, 3] and r["token_end"].tolist() == [1, 3, 4] and r["frame_pos"][:5].tolist() == [0, -1, 1, 2, -1]


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the inputs of the exact GPU comparisons: float32 and float64 chains agree on every one (no kernel involved)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(A.EXACT_CASES))
def test_exact_cases_do_not_depend_on_the_precision_of_the_chain(name):
    c = A.EXACT_CASES[name]()
    t64 = A.align_twin(c["y"], c["lens"], c["labels"], c["blank"], c["w"])
    t32 = A.align_twin(c["y"], c["lens"], c["labels"], c["blank"], c["w"], dtype=np.float32)
    n_aligned = 0
    for s, (a, b) in enumerate(zip(t64, t32)):
        assert a["status"] == b["status"]
        diff = int((a["state"] != b["state"]).sum())
        assert diff == 0, f"{name} stream {s}: the float32 chain leaves the float64 path in {diff} frames"
        if a["status"] == A.ALIGNED:
            n_aligned += 1
            validate_stream(a, c["lens"][s], c["labels"][s], c["blank"])
    assert n_aligned >= 1


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the C-ABI's host-side answers
# ---------------------------------------------------------------------------------------------------------------------------------
def test_align_workspace_query_and_limits():
    import kaldi_lstm_amd as k
    lib = k.load_library()
    for T, S, L in ((1000, 16, 150), (1000, 16, 0), (1, 1, 0), (300, 4, 31), (300, 4, 32), (65535, 1, 1023), (2047, 32, 1023), (50, 8, 5)):
        n = k.ctc_align_workspace_bytes(T, S, L)
        assert T * S * (2 * L + 1) // 4 <= n <= T * S * (2 * L + 1 + 8) + 4096, (T, S, L, n)
        assert n < k.ctc_workspace_bytes(T, S, L) or L == 0
    assert k.ctc_align_workspace_bytes(1000, 16, 150) * 20 < k.ctc_workspace_bytes(1000, 16, 150)
    sizes = [k.ctc_align_workspace_bytes(500, 8, L) for L in range(0, 1024, 31)]
    assert all(a <= b for a, b in zip(sizes[:-1], sizes[1:])) and sizes[0] < sizes[-1]
    sizes = [k.ctc_align_workspace_bytes(T, 8, 100) for T in (1, 10, 100, 1000, 8000)]
    assert all(a < b for a, b in zip(sizes[:-1], sizes[1:]))
    for T, S, L in ((2048, 32, 0), (1, 33, 0), (65536, 1, 0), (0, 1, 0), (10, 4, 1024), (10, 4, -1)):
        with pytest.raises(k.KlstmError) as ei:
            k.ctc_align_workspace_bytes(T, S, L)
        assert ei.value.status == 2 and b"klstm_ctc_align_workspace_bytes" in lib.klstm_last_error()
    # refused before anything touches the device: sizes first, then pointers
    n = None

    def call(T, S, K, stride):
        return lib.klstm_ctc_align(n, T, S, K, stride, n, n, n, 0, n, n, n, n, n, n, n, n, 0, n)
    assert call(10, 33, 8, 8) == 2
    assert call(10, 4, 40000, 40000) == 2
    assert call(10, 4, 1, 1) == 2 and b"klstm_ctc_align" in lib.klstm_last_error()
    assert call(0, 4, 8, 8) == 1
    assert call(10, 4, 8, 8) == 1 and b"null" in lib.klstm_last_error()


# ---------------------------------------------------------------------------------------------------------------------------------
# AlignCtcWholeUtterances hands alignments back in the order of the utterance list; SetTargetsFromAlignment fills the targets
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,sort,max_frames,lens", [
    (3, 1, 0, [5, 9, 0, 7, 9, 2, 30000]),            # the 30000-frame utterance and the empty one are skipped: no alignment, no targets
    (4, 0, 8, [5, 9, 3, 7, 9, 2, 8, 1, 6]),          # list order, two over the cap, one stream idle in the last minibatch
    (4, 1, 0, [6, 6, 2, 6, 9, 2, 6, 2]),             # ties keep the order of the list
    (1, 1, 0, [3, 1, 2]),
    (8, 1, 0, [4, 2]),
])
def test_alignments_come_back_in_utterance_order_and_fill_targets(S, sort, max_frames, lens):
    r = run_driver("order", S, sort, max_frames, ",".join(str(v) for v in lens))
    lines = r.stdout.split("\n")
    cap = max_frames if max_frames > 0 else 65535 // S
    utts = plain_utts(lens)
    _, skipped = R.batch_twin(utts, S, bool(sort), cap)
    assert [int(v) for v in lines[0].split()[1:3]] == [skipped, len(lens) - skipped]
    for i, n in enumerate(lens):
        targets, begins = ([int(v) for v in part.split(",")] if part else [] for part in lines[1 + i].split(";"))
        if 0 < n <= cap:
            assert targets == [i + 1] + [99] * (n - 1) and begins == utts[i][1]
        else:
            assert targets == [] and begins == []
