"""The references of the small CTC suite (tests/test_ctc_small_gpu.py), pinned without a GPU: truth64() of tests/ctc_ref.py against the
enumeration of all alignments, the exactly feasible utterances (one alignment: gamma is one-hot), the grid and the posteriors
themselves, and the kernel's recipe in numpy float32 (norm_twin) -- the yardstick of the device's bars -- against truth64 with its
pooled errors on record, next to what stock fp32 CTC delivers on the same utterances."""
import itertools

import numpy as np
import pytest
import torch

from tests import ctc_ref as R
from tests.margins import bound

GROUPS = pytest.mark.parametrize("K,blank", R.SMALL_GROUPS)


def enumerate_paths(y, labels, blank):
    """(-log p, gamma [T, K]) from ALL alignments of `labels` to the T frames of y [T, K] float64 (linear domain: tiny cases only)"""
    T, K = y.shape
    tot, occ = 0.0, np.zeros((T, K))
    for path in itertools.product(range(K), repeat=T):
        col = [k for k, _ in itertools.groupby(path)]
        if [k for k in col if k != blank] == list(labels):
            p = float(np.prod(y[np.arange(T), list(path)]))
            tot += p
            occ[np.arange(T), list(path)] += p
    return (-np.log(tot), occ / tot) if tot > 0 else (np.inf, occ)


def test_grid_counts_and_packing():
    for (K, blank), want in zip(R.SMALL_GROUPS, [135, 135, 135, 36, 36, 360, 360]):
        calls = list(R.small_grid(K, blank))
        seen, rejected = set(), 0
        for lens, labels in calls:
            assert len(lens) == len(labels) <= R.SMALL_S and lens.count(0) == 1 and labels[lens.index(0)] == []
            assert all(blank not in lab and all(0 <= c < K for c in lab) and len(lab) <= 3 for lab in labels)
            assert max(lens) == R.SMALL_T or len(lens) < 10
            seen |= {(n, tuple(lab)) for n, lab in zip(lens, labels) if n > 0}
            rejected += sum(R.infeasible(lens, labels, K, blank, R.SMALL_T))
        assert len(seen) == want == sum(len(lens) - 1 for lens, _ in calls)
        assert all(len(lens) == R.SMALL_S for lens, _ in calls[:-1])
        assert 0.15 * want < rejected < 0.3 * want                       # about a quarter: 30 of 135, 6 of 36, 84 of 360
        assert {n for n, _ in seen} == set(range(1, R.SMALL_T + 1))


def test_posterior_kinds():
    g = torch.Generator().manual_seed(1)
    for kind in ("flat", "peaked"):
        y = R.small_posteriors(kind, 9, 32, 4, g)
        assert y.dtype == torch.float32 and y.shape == (9, 32, 4) and bool((y > 0).all()) and bool((y <= 1).all())
        assert float((y.sum(-1) - 1).abs().max()) < 1e-6
    assert float(R.small_posteriors("peaked", 9, 32, 4, g).max(-1).values.median()) > 0.99
    y = R.small_posteriors("saturated", 9, 32, 4, g)
    assert bool(((y == 0.0) | (y == 1.0)).all()) and bool((y.sum(-1) == 1.0).all())
    assert bool((y.sum((0, 1)) > 0).all())                               # every class is the hot one somewhere


@GROUPS
@pytest.mark.parametrize("kind", ["flat", "peaked"])
def test_truth_equals_enumeration(K, blank, kind):
    """truth64 against brute_force on the raw posteriors, every utterance of the grid with T <= 5: the loss within 1e-9 relative, which
    streams are infeasible, and (T <= 4) gamma within 1e-9 of the alignments' own occupancy"""
    worst = checked = 0
    for c in R.small_group(K, blank, kind):
        yd = np.maximum(c["y"].numpy().astype(np.float64), R.FLT_MIN)
        for s, n in enumerate(c["lens"]):
            if not 0 < n <= 5:
                continue
            want = R.brute_force(yd[:n, s], c["labels"][s], blank)
            assert c["bad"][s] == np.isinf(want) == np.isinf(c["l64"][s])
            if c["bad"][s]:
                assert not c["d64"][:, s].any()
                continue
            err = abs(c["l64"][s] - want) / abs(want)
            worst, checked = max(worst, err), checked + 1
            assert err <= 1e-9, (c["lens"][s], c["labels"][s], c["l64"][s], want)
            if n <= 4:
                loss, gam = enumerate_paths(yd[:n, s], c["labels"][s], blank)
                assert abs(loss - want) <= 1e-12 * abs(want)
                assert np.abs((c["y"][:n, s].numpy().astype(np.float64) - c["d64"][:n, s]) - gam).max() <= 1e-9
            assert not c["d64"][n:, s].any()
    print(f"truth64 vs enumeration K={K} blank={blank} {kind}: {checked} feasible utterances, worst relative loss error {worst:.3g}", flush=True)
    assert checked >= (14 if K == 2 else 45)


@GROUPS
@pytest.mark.parametrize("kind", R.SMALL_KINDS)
def test_exactly_feasible_utterances(K, blank, kind):
    """len == L + repeats (and every L = 0 utterance): one single alignment, so gamma is exactly one-hot and the loss is the sum of that
    path's emissions -- also where the path runs through clamped zeros"""
    checked = 0
    for c in R.small_group(K, blank, kind):
        y64 = c["y"].numpy().astype(np.float64)
        for s, n in enumerate(c["lens"]):
            lab = c["labels"][s]
            path = R.single_path(lab, blank) if lab else [blank] * n
            if n == 0 or c["bad"][s] or len(path) != n:
                continue
            hot = np.zeros((n, K))
            hot[np.arange(n), path] = 1.0
            assert np.array_equal(c["d64"][:n, s], y64[:n, s] - hot), (n, lab)
            want = -np.log(np.maximum(y64[np.arange(n), s, path], R.FLT_MIN)).sum()
            assert abs(c["l64"][s] - want) <= 1e-12 * max(1.0, abs(want)), (n, lab, c["l64"][s], want)
            checked += 1
    assert checked >= 9 + (3 if K == 2 else 9)


def test_twin_takes_an_empty_label_sequence():
    y = torch.softmax(torch.randn(6, 5, generator=torch.Generator().manual_seed(2)), -1).numpy()
    loss, diff = R.norm_twin(y, [], 3)
    hot = np.zeros_like(y)
    hot[:, 3] = 1.0
    assert np.array_equal(diff, y - hot)
    assert abs(loss + np.log(y[:, 3].astype(np.float64)).sum()) <= 1e-6 * loss


@GROUPS
@pytest.mark.parametrize("kind", R.SMALL_KINDS)
def test_twin_under_the_bars(K, blank, kind):
    """norm_twin (L = 0 included) under the bars tests/test_ctc_small_gpu.py puts on the device, with the factor 4 replaced by 1 -- true by
    construction; what it puts on record through bound() is the SIZE of the yardstick, per group.  Asserted: on no group is the twin's
    diff further from truth64 than stock fp32 CTC (torch's float32 ctc_loss on the same utterances) is."""
    e_tw = r_tw = e_32 = r_32 = 0.0
    for c in R.small_group(K, blank, kind):
        e, r = R.pooled_errors(c["ltw"], c["dtw"], c["l64"], c["d64"], c["lens"], c["bad"])
        e_tw, r_tw = max(e_tw, e), max(r_tw, r)
        l32, d32 = R.oracle(c["y"], c["lens"], c["labels"], blank, torch.float32)
        e, r = R.pooled_errors(l32, d32, c["l64"], c["d64"], c["lens"], c["bad"])
        e_32, r_32 = max(e_32, e), max(r_32, r)
    print(f"small twin K={K} blank={blank} {kind}: diff twin {e_tw:.3g} stock fp32 {e_32:.3g} | loss twin {r_tw:.3g} stock fp32 {r_32:.3g}",
          flush=True)
    assert e_tw > 0 and r_tw > 0
    bound(e_tw, 1.0 * e_tw, "twin diff vs truth64 (bar: 1 x twin)")
    bound(r_tw, 1.0 * r_tw, "twin utt_loss vs truth64, relative to max(1, |truth|) (bar: 1 x twin)")
    bound(e_tw, e_32, "twin diff vs truth64 (bar: stock fp32)")
