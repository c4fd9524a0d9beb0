"""CTC on whole utterances, host side (no GPU): WholeUtteranceBatcher (include/klstm_trainer.hpp) against its numpy twin through
tests/cpp/ctc_test (whose build also shows that Ctc / TrainCtcWholeUtterances of include/klstm_nnet.hpp compile against the C-ABI), the
yardstick of tests/test_ctc_gpu.py pinned without torch (all alignments of a tiny case enumerated in float64), the kernel's recipe --
normalised log-domain recursions in float32, tests/ctc_ref.norm_twin -- against that yardstick under the GPU tests' bars, and the
host-side limits of the C-ABI."""

import numpy as np
import pytest
import torch

from tests import cpp_driver
from tests import ctc_ref as R



def build_ctc_driver():
    return cpp_driver.build("ctc_test")


def run_driver(*args, ok=True):
    return cpp_driver.run("ctc_test", *args, ok=ok)


# ---------------------------------------------------------------------------------------------------------------------------------
# WholeUtteranceBatcher
# ---------------------------------------------------------------------------------------------------------------------------------
def plain_utts(lens):
    """the utterances tests/cpp/ctc_test builds in its batcher mode"""
    out = []
    for i, n in enumerate(lens):
        f = (1000.0 * i + np.arange(n, dtype=np.float32)[:, None] + 0.25 * np.arange(3, dtype=np.float32)[None, :]).astype(np.float32)
        out.append((f, [i + j for j in range(i % 5)]))
    return out


@pytest.mark.parametrize("S,sort,max_frames,lens", [
    (3, 1, 0, [5, 9, 0, 7, 9, 2, 30000]),            # default cap 65535 / 3: the 30000-frame utterance and the empty one are skipped
    (4, 0, 8, [5, 9, 3, 7, 9, 2, 8, 1, 6]),          # list order, two over the cap, one stream idle in the last minibatch
    (4, 1, 0, [6, 6, 2, 6, 9, 2, 6, 2]),             # ties keep the order of the list; the last minibatch is full
    (1, 1, 0, [3, 1, 2]),
    (8, 1, 0, [4, 2]),                                # fewer utterances than streams
])
def test_whole_utterance_batcher_equals_twin(tmp_path, S, sort, max_frames, lens):
    out = str(tmp_path / "b.bin")
    r = run_driver("batcher", S, sort, max_frames, ",".join(str(v) for v in lens), out)
    nmb, done, skipped = (int(v) for v in r.stdout.split()[1:4])
    cap = max_frames if max_frames > 0 else 65535 // S
    want, want_skipped = R.batch_twin(plain_utts(lens), S, bool(sort), cap)
    assert nmb == len(want) and skipped == want_skipped and done == len(lens) - want_skipped
    raw = np.fromfile(out, dtype=np.int32)
    p, seen = 0, []
    for mb in want:
        T = int(raw[p]); p += 1
        assert T == mb["T"]
        assert raw[p:p + S].tolist() == mb["lens"]; p += S
        assert raw[p:p + S].tolist() == mb["index"]; p += S
        for s in range(S):
            L = int(raw[p]); p += 1
            assert raw[p:p + L].tolist() == mb["labels"][s]; p += L
        feat = raw[p:p + T * S * 3].view(np.float32).reshape(T * S, 3); p += T * S * 3
        assert feat.tobytes() == mb["feat"].tobytes()
        assert T == max(mb["lens"])
        seen += [i for i in mb["index"] if i >= 0]
    assert p == raw.size
    assert sorted(seen) == [i for i, n in enumerate(lens) if 0 < n <= cap]        # every utterance handed out exactly once


# ---------------------------------------------------------------------------------------------------------------------------------
# the yardstick, pinned without torch; the kernel's recipe under the GPU tests' bars
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("labels", [[], [1], [2, 1], [1, 1], [1, 2, 1], [2, 2, 1]])
def test_oracle_equals_enumeration(labels):
    rng = np.random.RandomState(len(labels) * 7 + sum(labels))
    T, K = 5, 3
    x = rng.randn(T, 1, K) * 1.5
    y = torch.softmax(torch.from_numpy(x).float(), -1)
    loss, diff = R.oracle(y, [T], [labels], 0)
    a64 = torch.log(torch.clamp_min(y[:, 0], R.FLT_MIN)).double().numpy()       # the recipe's own input: float32 logs, then float64

    def enum(a):                                                                 # log_softmax in front, as in the recipe
        p = np.exp(a - a.max(-1, keepdims=True))
        return R.brute_force(p / p.sum(-1, keepdims=True), labels, 0)
    want = enum(a64)
    assert R.infeasible([T], [labels], K, 0) == [not np.isfinite(want)]
    if not np.isfinite(want):
        assert loss[0] == 0.0 and not diff.any()                 # zero_infinity
        return
    assert abs(loss[0] - want) <= 1e-12 * max(1.0, want)
    num = np.zeros((T, K))                                       # d loss / d a by central differences of the enumeration
    h = 1e-6
    for t in range(T):
        for c in range(K):
            up, dn = a64.copy(), a64.copy()
            up[t, c] += h
            dn[t, c] -= h
            num[t, c] = (enum(up) - enum(dn)) / (2 * h)
    assert np.abs(diff[:, 0] - num).max() < 1e-8


def test_other_blank_equals_enumeration():
    rng = np.random.RandomState(3)
    y = torch.softmax(torch.from_numpy(rng.randn(5, 1, 3)).float(), -1)
    loss, _ = R.oracle(y, [5], [[0, 2]], 1)
    p = torch.softmax(torch.log(y[:, 0]).double(), -1).numpy()
    assert abs(loss[0] - R.brute_force(p, [0, 2], 1)) <= 1e-12 * loss[0]
    tw, _ = R.norm_twin(y[:, 0].numpy(), [0, 2], 1)
    assert abs(tw - loss[0]) <= 1e-6 * loss[0]


def test_normalised_recipe_meets_the_gpu_bars():
    """the recursion the kernel runs (numpy float32) against fp64, under the bars of tests/test_ctc_gpu.py: stock fp32 / 8 for diff,
    stock fp32 for the loss"""
    lens, labs = [300, 299, 250, 180, 120, 61, 30, 7], [40, 60, 33, 50, 60, 30, 29, 3]
    y, labels = R.make_case(1, 300, 48, 3.0, lens, labs, equal_labels=(5,))
    l64, d64 = R.oracle(y, lens, labels, 0)
    l32, d32 = R.oracle(y, lens, labels, 0, torch.float32)
    e_tw = e_32 = r_tw = r_32 = 0.0
    for s, n in enumerate(lens):
        ls, d = R.norm_twin(y[:n, s].numpy(), labels[s], 0)
        e_tw = max(e_tw, np.abs(d - d64[:n, s]).max())
        e_32 = max(e_32, np.abs(d32[:n, s] - d64[:n, s]).max())
        r_tw = max(r_tw, abs(ls - l64[s]) / l64[s])
        r_32 = max(r_32, abs(l32[s] - l64[s]) / l64[s])
    assert e_tw <= e_32 / 8 and r_tw <= r_32, (e_tw, e_32, r_tw, r_32)
    assert e_32 > 5e-4                                           # stock fp32 really is that far off (1.4e-3 measured)


def test_infeasible_matches_torch():
    lens, labs = [300, 299, 250, 180, 120, 58, 30, 2], [40, 60, 33, 50, 60, 30, 31, 3]
    y, labels = R.make_case(1, 300, 48, 3.0, lens, labs, equal_labels=(5,))
    a = torch.log(y).double()
    l = torch.nn.functional.ctc_loss(torch.log_softmax(a, -1), torch.tensor([c for lab in labels for c in lab]), torch.tensor(lens),
                                     torch.tensor(labs), blank=0, reduction="none")
    assert R.infeasible(lens, labels, 48, 0) == torch.isinf(l).tolist() == [False] * 5 + [True] * 3


# ---------------------------------------------------------------------------------------------------------------------------------
# the C-ABI's host-side answers
# ---------------------------------------------------------------------------------------------------------------------------------
def test_workspace_query_and_limits():
    import kaldi_lstm_amd as k
    lib = k.load_library()
    a, b = k.ctc_workspace_bytes(1000, 16, 150), k.ctc_workspace_bytes(1000, 16, 160)
    assert 2 * 1000 * 16 * 301 * 4 <= a <= 2 * 1000 * 16 * 304 * 4 + (1 << 20) and a < b
    assert k.ctc_workspace_bytes(2047, 32, 1023) < 1.1e9         # both chains' rows at the limits
    for T, S, L in ((2048, 32, 0), (1, 33, 0), (0, 1, 0), (10, 4, 1024), (10, 4, -1)):
        with pytest.raises(k.KlstmError) as ei:
            k.ctc_workspace_bytes(T, S, L)
        assert ei.value.status == 2 and b"klstm_ctc_workspace_bytes" in lib.klstm_last_error()
    # refused before anything touches the device: sizes first, then pointers
    assert lib.klstm_ctc_eval(None, 10, 33, 8, 8, None, None, None, 0, None, 8, None, None, None, 0, None) == 2
    assert lib.klstm_ctc_eval(None, 10, 4, 40000, 40000, None, None, None, 0, None, 40000, None, None, None, 0, None) == 2
    assert lib.klstm_ctc_eval(None, 10, 4, 8, 8, None, None, None, 0, None, 8, None, None, None, 0, None) == 1
