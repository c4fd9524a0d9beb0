"""The yardsticks of the small n-best risk suite (tests/test_ctc_mbr_small_gpu.py), pinned without a GPU: objective64 of
tests/ctc_mbr_ref.py against the enumeration of all frame paths on COMPLETE lists (every feasible labelling, so that P is the true
posterior) and against central differences of the objective, truth64 against the torch oracle (a guard against a mix-up of
conventions: the two differ by the row renormalisation), the float32 twin of the documented recipe with its pooled errors on record,
and the conditions of the grid itself -- how many streams are counted, rejected and idle, how many entries are dropped, that no
counted stream has equal costs throughout, that flat posteriors leave P far from one-hot."""
import itertools

import numpy as np
import pytest
import torch

from tests import ctc_mbr_ref as M
from tests import ctc_ref as R

GROUPS = pytest.mark.parametrize("K,blank", R.SMALL_GROUPS)
COMPLETE_GROUPS = [(K, blank) for K, blank in R.SMALL_GROUPS if K in M.COMPLETE_T]


@pytest.mark.parametrize("kind", R.SMALL_KINDS)
@pytest.mark.parametrize("K,blank", COMPLETE_GROUPS)
def test_truth_equals_path_enumeration_on_complete_lists(K, blank, kind):
    """K = 3 at T = 1..4 and K = 2 at T = 1..5, the list every feasible labelling (15 at T = 4, K = 3): risk, post and every element
    of diff of objective64 within 1e-9 of the sums over all K^T paths, at kappa = 1 and, the paths pooled per labelling, at 0.5 and 4"""
    c = M.complete_case(K, blank, kind)
    assert c["lens"] == list(range(1, M.COMPLETE_T[K] + 1)) and max(c["counts"]) == (15 if K == 3 else 4)
    assert c["t64"]["status"] == ["counted"] * len(c["lens"]) and not any(any(d) for d in c["t64"]["dropped"])
    worst = 0.0
    for s, n in enumerate(c["lens"]):
        y = c["yd"][:n, s]
        for kappa in (1.0, 0.5, 4.0):
            o = M.objective64(y, c["lists"][s], c["costs"][s], None, blank, kappa, 0.0)
            e = c["enum"][s] if kappa == 1.0 else M.enumerate_objective(y, c["lists"][s], c["costs"][s], blank, kappa)
            # completeness, on the inputs: no path collapses to a labelling outside the list, and the listed ones carry all the mass
            rows = float(np.prod(y.sum(-1)))
            assert e["missing"] == 0.0 and abs(e["total"] - rows) <= 1e-12 * rows
            assert abs(float(np.exp(o["logp"]).sum()) - rows) <= 1e-12 * rows, "the list does not hold every labelling"
            err = max(abs(o["risk"] - e["risk"]), float(np.abs(o["post"] - e["post"]).max()), float(np.abs(o["diff"] - e["diff"]).max()))
            worst = max(worst, err)
            assert err <= 1e-9, (n, kappa, err)
            if kappa == 1.0:
                assert np.array_equal(c["t64"]["diff"][:n, s], o["diff"]) and c["t64"]["risk"][s] == o["risk"]
    # the formula of the issue, path by path, at kappa = 1 on the longest stream: R = E[W], diff(t, k) = E[(W - R) [path_t = k]]
    s, n = len(c["lens"]) - 1, c["lens"][-1]
    y, index = c["yd"][:n, s], {tuple(l): q for q, l in enumerate(c["lists"][s])}
    paths = list(itertools.product(range(K), repeat=n))
    pr = np.array([np.prod(y[np.arange(n), list(p)]) for p in paths])
    w = np.array([c["costs"][s][index[tuple(k for k in (k for k, _ in itertools.groupby(p)) if k != blank)]] for p in paths], dtype=np.float64)
    risk = float((pr * w).sum() / pr.sum())
    d = np.zeros((n, K))
    for p, a, b in zip(paths, pr / pr.sum(), w):
        d[np.arange(n), list(p)] += a * (b - risk)
    assert abs(risk - c["t64"]["risk"][s]) <= 1e-9 and np.abs(d - c["t64"]["diff"][:n, s]).max() <= 1e-9
    print(f"objective64 vs path enumeration K={K} blank={blank} {kind}: worst {worst:.3g}", flush=True)


@pytest.mark.parametrize("kappa,lam", [(1.0, 0.0), (0.5, 0.3)])
@pytest.mark.parametrize("K,blank", [(3, 1), (4, 0)])
def test_truth_diff_is_the_gradient_with_respect_to_the_softmax_input(K, blank, kappa, lam):
    """central differences of risk + lam * ref_loss over a float64 softmax input, on the incomplete small_list: with y = softmax(a) in
    float64 the formula is the exact gradient (step 1e-5, agreement 1e-7, largest entry > 1e-3: the figures of tests/test_ctc_mmi.py)"""
    n = 5
    entries = M.small_list(K, blank)
    classes = [c for c in range(K) if c != blank]
    ref = [classes[0], classes[-1]]
    costs = [int(M.B.levenshtein(e, ref)) for e in entries]
    assert not any(R.infeasible([n] * len(entries), entries, K, blank)) and len(set(costs)) > 1
    a = np.random.RandomState(10 * K + blank).randn(n, K)

    def f(a):
        y = np.exp(a - a.max(1, keepdims=True))
        y /= y.sum(1, keepdims=True)
        o = M.objective64(y, entries, costs, ref, blank, kappa, lam)
        return o["risk"] + lam * o["ref_loss"], o
    _, o = f(a)
    h, worst = 1e-5, 0.0
    for t, k in itertools.product(range(n), range(K)):
        d = np.zeros_like(a)
        d[t, k] = h
        worst = max(worst, abs((f(a + d)[0] - f(a - d)[0]) / (2 * h) - o["diff"][t, k]))
    print(f"objective64 diff against central differences, K {K} kappa {kappa} lam {lam}: {worst:.3g} (largest entry "
          f"{np.abs(o['diff']).max():.3g})", flush=True)
    assert worst <= 1e-7 and np.abs(o["diff"]).max() > 1e-3


def test_truth_stays_near_the_torch_oracle():
    """truth64 (raw posteriors) against oracle() (float32 logarithms, rows renormalised) on one flat call with every entry feasible:
    the two differ by the renormalisation of rows whose float32 sum is not 1, far below 1e-5"""
    K, blank, S = 4, 0, 6
    y = R.small_posteriors("flat", R.SMALL_T, S, K, torch.Generator().manual_seed(5))
    lens = [9, 9, 8, 7, 6, 5]
    refs = [[1, 2], [3], [], [2, 2], [1, 2, 3], [3, 1]]
    c = M.small_call(y, lens, refs, K, blank, 0.5, 0.3)
    assert c["t64"]["status"] == ["counted"] * S and not any(any(d) for d in c["t64"]["dropped"])
    o = M.oracle(y, lens, c["lists"], c["costs"], refs, blank, c["kappa"], c["lam"])
    e = max(float(np.abs(o["diff"] - c["t64"]["diff"]).max()), float(np.abs(o["risk"] - c["t64"]["risk"]).max()),
            float(np.abs(o["ref_loss"] - c["t64"]["ref_loss"]).max()),
            max(float(np.abs(np.array(o[key][s]) - np.array(c["t64"][key][s])).max()) for s in range(S) for key in ("post", "logp")))
    print(f"truth64 against the torch oracle: {e:.3g} (largest diff entry {np.abs(o['diff']).max():.3g})", flush=True)
    assert e <= 1e-5 and np.abs(o["diff"]).max() > 1e-3


def grid_status(K, blank, lam):
    """(status, dropped, lists, costs) of every call of the grid with the reference in use (lam > 0) or not, from labels alone"""
    entries = M.small_list(K, blank)
    N = len(entries)
    out = []
    for lens, refs in R.small_grid(K, blank):
        lists = [entries] * len(lens)
        costs = [[int(M.B.levenshtein(e, r)) for e in entries] for r in refs]
        st, dr = M.statuses(lens, lists, costs, [N] * len(lens), refs, K, blank, R.SMALL_T, N, M.SMALL_MAX_LEN, lam, stride=M.SMALL_STRIDE)
        out.append((st, dr, lens, costs))
    return out


# K: (calls over both passes, N, counted / rejected / idle with the reference in use, counted without it, idle over both passes,
#     dropped entries and entries of the counted streams over both passes)
GRID = {3: (10, 7, 105, 30, 135, 10, 112, 1680), 2: (4, 4, 30, 6, 36, 4, 38, 264), 4: (24, 16, 276, 84, 360, 24, 970, 10176)}


@GROUPS
def test_conditions_of_the_grid(K, blank):
    """on the reference alone: the figures of the grid with the reference in use on every call and on none"""
    calls, N, counted, rejected, counted0, idle, drops, entries = GRID[K]
    assert len(M.small_list(K, blank)) == N and len({tuple(e) for e in M.small_list(K, blank)}) == N
    assert [] in M.small_list(K, blank)                                          # the empty labelling is in every list
    with_ref, without = grid_status(K, blank, 0.3), grid_status(K, blank, 0.0)
    assert len(with_ref) + len(without) == calls

    def count(passes, what):
        return sum(st.count(what) for st, _, _, _ in passes)
    assert (count(with_ref, "counted"), count(with_ref, "rejected")) == (counted, rejected)
    assert count(without, "counted") == counted0 and count(without, "rejected") == 0
    assert count(with_ref, "idle") + count(without, "idle") == idle
    assert count(with_ref + without, "skipped") == 0
    seen = live = 0
    for st, dr, lens, costs in with_ref + without:
        for s in range(len(lens)):
            if st[s] != "counted":
                continue
            seen, live = seen + sum(dr[s]), live + len(dr[s])
            kept = {costs[s][q] for q in range(N) if not dr[s][q]}
            assert len(kept) > 1, "a counted stream whose live costs are all equal"
            assert not dr[s][0]                                                  # the empty labelling is never dropped
    print(f"small n-best grid K={K} blank={blank}: N {N}; with the reference {counted} counted {rejected} rejected; without {counted0} "
          f"counted; {idle} idle and {seen} of {live} entries dropped over both passes", flush=True)
    assert (seen, live) == (drops, entries)


@pytest.mark.parametrize("kind", R.SMALL_KINDS)
@GROUPS
def test_groups_and_their_twin(K, blank, kind):
    """the groups as the device sees them ((kappa, lam) cycling): the statuses are those the grid predicts, every group has counted and
    rejected streams, dropped entries inside counted streams and, under flat posteriors, lists whose P is far from one-hot; the twin's
    pooled errors against truth64 are finite and on record"""
    group = M.small_group(K, blank, kind)
    scales = M.small_scales(K, blank)
    assert [(c["kappa"], c["lam"]) for c in group] == [(float(np.float32(a)), float(np.float32(b))) for a, b in scales]
    first = 1 if K == 2 else 0                                                   # see small_scales(): K = 2 has two calls
    assert scales == [M.SMALL_SCALES[(first + i) % 4] for i in range(len(group))] and len(group) == GRID[K][0] // 2
    counted = rejected = drops = spread = 0
    e_tw = r_tw = l_tw = 0.0
    for c, (lens, refs) in zip(group, R.small_grid(K, blank)):
        t, tw = c["t64"], c["tw"]
        assert c["lens"] == lens and c["refs"] == refs and c["counts"] == [c["N"]] * len(lens)
        bad = R.infeasible(lens, refs, K, blank, R.SMALL_T)
        want = ["idle" if n == 0 else "rejected" if c["lam"] > 0 and bad[s] else "counted" for s, n in enumerate(lens)]
        assert t["status"] == want == tw["status"] and t["dropped"] == tw["dropped"]
        for s, n in enumerate(lens):
            if want[s] != "counted":
                assert not t["diff"][:, s].any() and not tw["diff"][:, s].any() and t["risk"][s] == 0 and t["live"][s] == []
                continue
            assert t["dropped"][s] == R.infeasible([n] * c["N"], c["lists"][s], K, blank)
            drops += sum(t["dropped"][s])
            assert abs(sum(t["post"][s]) - 1.0) <= 1e-12 and not t["diff"][n:, s].any() and not tw["diff"][n:, s].any()
            if c["lam"] == 0:
                assert np.abs(t["diff"][:n, s].sum(-1)).max() <= 1e-12 * max(1.0, c["kappa"])
            spread += len(t["post"][s]) > 1 and sorted(t["post"][s])[-2] > 1e-2
        counted, rejected = counted + want.count("counted"), rejected + want.count("rejected")
        e, r, l, _ = M.pooled(tw, t, lens)
        e_tw, r_tw, l_tw = max(e_tw, e), max(r_tw, r), max(l_tw, l)
    print(f"small n-best twin K={K} blank={blank} {kind}: {counted} counted {rejected} rejected {drops} dropped entries, {spread} streams "
          f"with a second P > 1e-2 | twin vs truth64: diff {e_tw:.3g} risk {r_tw:.3g} logp {l_tw:.3g}", flush=True)
    assert np.isfinite([e_tw, r_tw, l_tw]).all() and e_tw > 0
    assert counted > 20 and rejected > 5 and drops >= 1
    if kind == "flat":
        assert spread >= 10
