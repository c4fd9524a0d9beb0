"""Transducer forced alignment on the GPU (rnnt_align: krnnt_align, krnnt_band_align) against tests/rnnt_align_ref.py, over the table of
tests/test_rnnt_band_gpu.py (every case as the full lattice and in its band) and four more shapes for the bit words.  Parity per stream:
the bar of tests/test_rnnt_gpu.py, max(4 x the float32 twin, 2^-22) against float64, for the score, the label log-probabilities and the
GPU's path rescored on the float64 planes; the frames equal the reference's wherever its smallest decision margin on the best path is at
least 1e-3 (the candidates of the kernel and of float64 agree to about 1e-5).  bf16: 2 e_q, as tests/test_rnnt_band_bf16_gpu.py.  The
measured fractions: profiles/rnnt_align_margins.json, DESIGN.md 4zd."""
import functools

import numpy as np
import pytest
import torch

from tests import rnnt_align_ref as ref
from tests.margins import bound
from tests.rnnt_ref import rel_err
from tests.test_rnnt_band_gpu import CASES, band_rule, problem
from tests.test_rnnt_gpu import FLOOR, MARGIN

pytestmark = pytest.mark.gpu
f32 = np.float32
SENTINEL, MIN_MARGIN = -7, 1e-3
# (T, Umax) = (6, 63): one full word of decisions; (6, 64): one bit into the second word; (3, 130): three waves; (6200, 1): the words of
# neither kernel fit its LDS and go through the workspace.  The last entry is the seed, chosen on the CPU for a margin above 1e-3.
WORDS = [(6, 63, 5, 16, 1, 64, "zero", None, 0, 0), (6, 64, 5, 16, 1, 64, "linear", None, 0, 0), (3, 130, 5, 16, 1, 64, "linear", None, 0, 0),
         (6200, 1, 5, 16, 1, 2, "zero", None, 0, 0)]
TABLE = [(c, banded) for c in CASES + WORDS for banded in (False, True)]
name = lambda c: "T%d-U%d-V%d-J%d-S%d-R%d-%s-l%s-b%d" % c[:9]


@functools.lru_cache(maxsize=None)
def inputs(case):
    """problem()'s first eight for its table; one full-length stream for WORDS"""
    if len(case) == 9:
        return problem(*case)[:8]
    T, Umax, V, J, S, R, kind = case[:7]
    rng = np.random.RandomState(case[9] + T)
    enc, pred = rng.randn(T, J).astype(f32), rng.randn(Umax + 1, J).astype(f32)
    W, b = rng.uniform(-0.3, 0.3, (V, J)).astype(f32), rng.uniform(-0.3, 0.3, V).astype(f32)
    band = np.array([[0] * T if kind == "zero" else band_rule(T, Umax, R, (R - 1) // 2)], np.int32)
    return enc, pred, W, b, [T], [[int(v) for v in rng.randint(1, V, Umax)]], 0, band


@functools.lru_cache(maxsize=None)
def reference(case, banded, bf16=False):
    enc, pred, W, b, lens, labels, blank, band = inputs(case)
    kw = dict(band=band, R=case[5]) if banded else {}
    (truth, pl), (twin, _) = [ref.align(enc, pred, W, b, lens, labels, blank, dt, bf16=bf16, **kw) for dt in (torch.float64, torch.float32)]
    return truth, twin, pl


def launch(inputs, band=None, R=None, **kw):
    import kaldi_lstm_amd as k
    enc, pred, W, b, lens, labels, blank = inputs
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    if band is not None:
        kw.update(band_lo=d(band.astype(np.int32)), R=R)
    res = k.rnnt_align(d(enc), d(pred), d(W), d(b), lens, labels, blank=blank, want_logp=True, **kw)
    off = np.cumsum([0] + [len(y) for y in labels])
    fr, lp = res["frames"].cpu().numpy(), res["logp"].cpu().numpy()
    return [(fr[i:j].tolist(), lp[i:j]) for i, j in zip(off, off[1:])], res["score"].cpu().numpy(), res


def run(case, banded, **kw):
    p = inputs(case)
    return launch(p[:7], p[7] if banded else None, case[5], **kw)


def check_stream(tag, fr, lp, score, truth, twin, planes, Ts, band_row=None, R=None):
    tscore, tframes, tlogp, margin = truth
    assert len(fr) == len(tframes) and fr == sorted(fr) and all(0 <= f < Ts for f in fr), tag
    e32 = rel_err(twin[0], tscore)
    figures = [("score", rel_err(score, tscore), e32), ("path", rel_err(ref.rescore(*planes, fr, band_row, R), tscore), e32)]
    if tframes:
        figures.append(("logp", rel_err(lp, tlogp), rel_err(twin[2], tlogp)))
    for what, err, twin_err in figures:
        print(f"{tag} {what}: {err:.3g} (twin {twin_err:.3g}, margin {margin:.3g})", flush=True)
        bound(err, max(MARGIN * twin_err, FLOOR), what)
    assert margin < MIN_MARGIN or fr == tframes, (tag, margin)


@pytest.mark.parametrize("case,banded", TABLE, ids=lambda v: name(v) if isinstance(v, tuple) else ("band" if v else "full"))
def test_align_against_float64(case, banded):
    lens, band = inputs(case)[4], inputs(case)[7]
    truth, twin, planes = reference(case, banded)
    streams, score, _ = run(case, banded)
    for s, Ts in enumerate(lens):
        check_stream("%s s%d" % (name(case), s), *streams[s], score[s], truth[s], twin[s], planes[s], Ts, band[s] if banded else None, case[5])


@pytest.mark.parametrize("case", CASES, ids=name)
def test_bf16_score_against_float64(case):
    truth, quantised = reference(case, True)[0], reference(case, True, True)[0]
    streams, score, _ = run(case, True, precision="bf16")
    lens = inputs(case)[4]
    for s, Ts in enumerate(lens):
        fr = streams[s][0]
        assert len(fr) == len(truth[s][1]) and fr == sorted(fr) and all(0 <= f < Ts for f in fr)
        eq = rel_err(quantised[s][0], truth[s][0])
        bar = 2.0 * eq if eq > 0 else max(MARGIN * rel_err(reference(case, True)[1][s][0], truth[s][0]), FLOOR)
        bound(rel_err(score[s], truth[s][0]), bar, "score s%d (e_q %.3g)" % (s, eq))


def test_bf16_and_f32_agree_where_the_logits_are_exact():
    """the saturated construction of tests/test_rnnt_band_bf16_gpu.py (h = +-1, W and b in k / 64): the same frames and the f32 bar"""
    T, Umax, V, J, R = 17, 5, 17, 48, 8
    rng = np.random.RandomState(11)
    enc, pred = rng.choice([-12.0, 12.0], (T, J)).astype(f32), rng.choice([-1.0, 0.0, 1.0], (Umax + 1, J)).astype(f32)
    W, b = (rng.randint(-32, 33, (V, J)) / 64.0).astype(f32), (rng.randint(-32, 33, V) / 64.0).astype(f32)
    inputs, band = (enc, pred, W, b, [T], [[int(v) for v in rng.randint(1, V, Umax)]], 0), np.zeros((1, T), np.int32)
    (truth, planes), (twin, _) = [ref.align(*inputs, dt, band=band, R=R) for dt in (torch.float64, torch.float32)]
    assert truth[0][3] >= MIN_MARGIN
    for precision in ("bf16", "f32"):
        streams, score, _ = launch(inputs, band, R, precision=precision)
        check_stream("saturated " + precision, *streams[0], score[0], truth[0], twin[0], planes[0], T, band[0], R)


@pytest.mark.parametrize("banded", [False, True], ids=["full", "band"])
def test_long_lattice(banded):
    rng = np.random.RandomState(5)
    T, U, J, V, R = 400, 60, 16, 4, 8
    enc, pred = rng.randn(T, J).astype(f32), rng.randn(U + 1, J).astype(f32)
    W, b = rng.uniform(-0.3, 0.3, (V, J)).astype(f32), rng.uniform(-0.3, 0.3, V).astype(f32)
    inputs, band = (enc, pred, W, b, [T], [[int(v) for v in rng.randint(1, V, U)]], 0), np.array([band_rule(T, U, R, 3)], np.int32) if banded else None
    (truth, planes), (twin, _) = [ref.align(*inputs, dt, band=band, R=R) for dt in (torch.float64, torch.float32)]
    streams, score, _ = launch(inputs, band, R)
    check_stream("long", *streams[0], score[0], truth[0], twin[0], planes[0], T, None if band is None else band[0], R)


def test_the_contract():
    """at most one stream of the table is under the margin; runs and company leave the bits alone; rejected and idle streams"""
    import kaldi_lstm_amd as k
    under = [(name(c), bd, s) for c, bd in TABLE for s, r in enumerate(reference(c, bd)[0]) if r is not None and r[3] < MIN_MARGIN]
    assert len(under) <= 1, under
    case = (17, 8, 17, 48, 3, 4, "frames", None, 0)
    T, Umax, V, J, S, R = case[:6]
    enc, pred, W, b, lens, labels, blank, band = inputs(case)
    bits = lambda r: [r[2][n].cpu().numpy().view(np.int32).tolist() for n in ("frames", "logp", "score")]
    for banded in (False, True):
        one, two = run(case, banded), run(case, banded)
        assert bits(one) == bits(two), "two runs differ"
        alone = launch((enc.reshape(T, S, J)[:, 0], pred.reshape(Umax + 1, S, J)[:, 0], W, b, lens[:1], labels[:1], blank), band[:1] if banded else None, R)
        assert [v[:len(w)] for v, w in zip(bits(one), bits(alone))] == bits(alone), "stream 0 depends on its company"
    # stream 0 runs; 1: a label equal to blank; 2: an invalid band (u0(0) = 1); 3: idle
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    lens4, labels4, rows = [9, 9, 9, 0], [[1, 2, 3], [1, 0, 2], [2, 1, 4], [3]], [band_rule(9, 3, 2, 0)] * 4
    rows[2] = [1] + rows[2][1:]
    rng = np.random.RandomState(3)
    args = [d(rng.randn(9 * 4, 16).astype(f32)), d(rng.randn(4 * 4, 16).astype(f32)), d(rng.uniform(-0.3, 0.3, (5, 16)).astype(f32)), d(np.zeros(5, f32))]
    lib, (lab, off, _) = k.load_library(), k.ctc.pack_labels(labels4, "cuda")
    fr, lp, sc = torch.full((10,), SENTINEL, dtype=torch.int32, device="cuda"), torch.full((10,), float(SENTINEL), device="cuda"), torch.full((4,), 1.0, device="cuda")
    nbytes = k.rnnt_align_workspace_bytes(9, 4, 3, 16, 5, R=2)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    assert lib.krnnt_band_align(args[0].data_ptr(), 16, args[1].data_ptr(), 16, args[2].data_ptr(), args[3].data_ptr(), 9, 4, 3, 16, 5, d(np.array(lens4, np.int32)).data_ptr(),
                                lab.data_ptr(), off.data_ptr(), 0, 2, d(np.array(rows, np.int32)).data_ptr(), 0, fr.data_ptr(), lp.data_ptr(), sc.data_ptr(), ws.data_ptr(), nbytes, None) == 0
    assert sc.tolist()[1:] == [0.0, 0.0, 0.0] and sc[0] < 0 and (fr[3:] == SENTINEL).all() and (lp[3:] == SENTINEL).all() and (fr[:3] >= 0).all()
    again = k.rnnt_band_from_frames(lens, labels, R, frames=run(case, False)[2]["frames"])
    assert again.shape == band.shape and not (again.cpu().numpy() == -1).any()
