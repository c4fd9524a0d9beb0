"""Minimum expected token error over CTC n-best lists, host side (no GPU): the oracle that the GPU tests are held against
(tests/ctc_mbr_ref.py) is pinned by torch autograd of the objective itself and by a brute-force case, the status rules are spelled
out, and the library carries the entry with its limits."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import cpp_driver
from tests import ctc_mbr_ref as M
from tests import ctc_ref as R


def build_ctc_mbr_driver():
    return cpp_driver.build("ctc_mbr_test")


def run_driver(*args, ok=True):
    return cpp_driver.run("ctc_mbr_test", *args, ok=ok)


def autograd_objective(y, n, labs, costs, ref, blank, kappa, lam):
    """R + lam * loss_ref of one stream by torch autograd in float64 -> (R, gradient with respect to the log posteriors [n, K])"""
    a = torch.log(torch.clamp_min(y[:n], R.FLT_MIN)).double().requires_grad_()
    sm = F.log_softmax(a, -1)[:, None]

    def loss(lab):
        return F.ctc_loss(sm, torch.tensor([lab], dtype=torch.long).reshape(1, -1), torch.tensor([n]), torch.tensor([len(lab)]), blank=blank,
                          reduction="none")[0]
    l = torch.stack([-loss(lab) for lab in labs])
    P = torch.softmax(kappa * l, 0)
    risk = (P * torch.tensor(costs, dtype=torch.float64)).sum()
    obj = risk + (lam * loss(ref) if lam > 0 else 0.0)
    obj.backward()
    return float(risk.detach()), a.grad.numpy()


@pytest.mark.parametrize("kappa,lam", [(1.0, 0.0), (0.5, 0.3)])
def test_oracle_diff_is_the_autograd_gradient_of_the_objective(kappa, lam):
    lens = [120, 97, 61]
    c = M.make_case(1, 120, 24, lens, [12, 9, 7])
    assert sum(len(set(w)) > 1 for w in c["costs"]) >= 2, c["costs"]
    o = M.oracle(c["y"], lens, c["lists"], c["costs"], c["refs"], 0, kappa, lam)
    worst = 0.0
    for s, n in enumerate(lens):
        risk, g = autograd_objective(c["y"][:, s], n, c["lists"][s], c["costs"][s], c["refs"][s], 0, kappa, lam)
        assert abs(risk - o["risk"][s]) <= 1e-12 * max(1.0, risk)
        worst = max(worst, float(np.abs(g - o["diff"][:n, s]).max()))
        assert not o["diff"][n:, s].any()
    print(f"oracle diff vs autograd: {worst:.3g} (largest entry {np.abs(o['diff']).max():.3g})", flush=True)
    assert worst <= 1e-7
    assert np.abs(o["diff"]).max() > 1e-3


def test_brute_force_list_of_every_labelling():
    """T = 4, K = 3: the list is every labelling with a non-zero probability, so P (at kappa 1) is the true posterior over labellings"""
    T, K, blank = 4, 3, 0
    y = torch.softmax(torch.randn(T, 1, K, generator=torch.Generator().manual_seed(3)) * 1.5, -1)
    # the posteriors as the oracle reads them: float32 logarithms, renormalised in float64
    y64 = torch.softmax(torch.log(torch.clamp_min(y[:, 0], R.FLT_MIN)).double(), -1).numpy()
    labs = [list(l) for n in range(T + 1) for l in itertools.product((1, 2), repeat=n)]
    labs = [l for l in labs if not R.infeasible([T], [l], K, blank)[0]]
    brute = np.array([-R.brute_force(y64, l, blank) for l in labs])
    assert abs(np.exp(brute).sum() - 1.0) < 1e-12, "the list does not hold every labelling"
    ref = [1, 2]
    costs = [int(M.B.levenshtein(l, ref)) for l in labs]
    o = M.oracle(y, [T], [labs], [costs], [ref], blank, 1.0, 0.0)
    assert np.abs(np.array(o["logp"][0]) - brute).max() < 1e-12
    assert np.abs(np.array(o["post"][0]) - np.exp(brute)).max() < 1e-12
    assert abs(o["risk"][0] - float((np.exp(brute) * costs).sum())) < 1e-12
    assert np.abs(o["diff"][:, 0].sum(-1)).max() < 1e-12          # the risk part sums to 0 over the classes of a row


def test_statuses():
    K, T, N = 8, 10, 3
    lists = [[[1, 2], [1], []],            # counted, nothing dropped (an empty labelling is legal)
             [[1, 2], [0, 1], [9]],        # a blank inside, a label outside [0, K): dropped
             [[1, 1, 1], [1, 2, 3, 4]],    # lens 4: three equal labels need 5 frames, four labels fit
             [[1] * 11],                   # longer than max_len
             [[1, 2]],                     # a cost of -1
             [[1, 2]],                     # idle
             [[1, 2]],                     # lens outside [0, T]
             [[1, 2]],                     # count outside [0, N]
             [],                           # count 0
             [[1, 2]]]                     # a reference with the blank in it
    costs = [[0, 1, 2], [0, 1, 1], [2, 0], [3], [-1], [0], [0], [0], [], [0]]
    counts = [3, 3, 2, 1, 1, 1, 1, 4, 0, 1]
    lens = [10, 10, 4, 10, 10, 0, 11, 10, 10, 10]
    refs = [[1, 2]] * 9 + [[1, 0]]
    st, dr = M.statuses(lens, lists, costs, counts, refs, K, 0, T, N, 10, 0.5)
    assert st == ["counted", "counted", "counted", "skipped", "skipped", "idle", "rejected", "rejected", "skipped", "rejected"]
    assert dr[0] == [False, False, False] and dr[1] == [False, True, True] and dr[2] == [True, False] and dr[3] == [True]
    st0, _ = M.statuses(lens, lists, costs, counts, refs, K, 0, T, N, 10, 0.0)
    assert st0[9] == "counted"             # without a CTC term the reference is not looked at


def test_abi_exports_and_limits():
    import kaldi_lstm_amd as k
    lib = k.load_library()
    assert hasattr(lib, "klstm_ctc_mbr_eval") and hasattr(lib, "klstm_ctc_mbr_workspace_bytes")
    q = lib.klstm_ctc_mbr_workspace_bytes
    at = [(2047, 32, 16, 1023, 1), (65535, 1, 1, 0, 0), (1, 1, 16, 1023, 0)]
    for a in at:
        assert q(*a) > 0, a
    beyond = [(2048, 32, 16, 1023, 1), (10, 33, 4, 10, 0), (10, 4, 17, 10, 0), (10, 4, 0, 10, 0), (10, 4, 4, 1024, 0), (0, 4, 4, 10, 0),
              (10, 4, 4, -1, 0)]
    for a in beyond:
        assert q(*a) == 0 and b"klstm_ctc_mbr_workspace_bytes" in lib.klstm_last_error(), a
    # the rows of both chains of every entry: 2 * T*S * (N + ref) * (2 L + 1 rounded up to 4) floats and a bounded head
    T, S, N, L = 1000, 16, 8, 150
    rows = 2 * T * S * (N + 1) * 304 * 4
    assert rows <= q(T, S, N, L, 1) <= rows + (8 << 20)
    assert q(T, S, N, L, 1) > q(T, S, N, L, 0) > q(T, S, N, L - 1, 0)
    with pytest.raises(k.KlstmError) as ei:
        k.ctc_mbr_workspace_bytes(10, 4, 17, 10)
    assert ei.value.status == 2


def test_cpp_driver_builds():
    r = run_driver(ok=False)
    assert r.returncode == 2 and "usage: ctc_mbr_test" in r.stderr
