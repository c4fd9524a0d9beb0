"""klstm_ctc_mmi_eval on the device (kaldi_lstm_amd.ctc_mmi_eval) against the float64 recursion of tests/ctc_mmi_ref.py.
THE BAR, per call: max |diff - truth64| over the counted rows and max |loss - truth64| / max(1, |loss|) are each at most 4 x the same
error of plain32 (the float32 log-domain recursion of ctc_mmi_ref on the same inputs; 4: the margin of tests/test_ctc_small_gpu.py),
floored at 2^-21 (eight float32 roundings of a value <= 1).  Measured ratios: profiles/ctc_mmi_parity_margins.json.
PLANS.  The denominator has ONE launch plan (one workgroup of 256 threads per chain, rows in LDS); the reference chain has the five of
klstm_ctc_eval, chosen by the label capacity that follows from the workspace's size.  All outputs are byte-equal between them."""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

import kaldi_lstm_amd as k
from kaldi_lstm_amd.binding import load_library
from tests import ctc_mmi_ref as M
from tests import ctc_ref as R
from tests.margins import bound

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -21
GRID_T = (1, 2, 3, 5, 9)
# (K, blank, language models, column window (pad, offset) or None)
GRID = [(3, 0, ("unigram", "bigram"), None), (3, 1, ("unigram", "bigram"), (5, 1)), (3, 2, ("bigram",), None),
        (4, 0, ("trigram", "lexicon"), None), (5, 0, ("unigram", "bigram", "lexicon"), (3, 3)), (7, 3, ("bigram", "lexicon"), (1, 1))]
KINDS = ("flat", "peaked", "saturated")


@functools.lru_cache(maxsize=None)
def device_lm(kind, K, blank):
    lm = M.make_lm(kind, K, blank)
    dlm = k.CtcLabelLm(*lm)
    return lm, k.CtcMmiDenominator(dlm, blank=blank)


def grid_calls(K, blank):
    """references of length 0..3 over three non-blank classes (two at K = 3), repeats included, at every length of GRID_T: calls of up to
    31 utterances and one idle stream, T = 9 rows each (so shorter utterances have padding rows)"""
    classes = [c for c in range(K) if c != blank]
    classes = [classes[0], classes[-1]] if K == 3 else [classes[0], classes[1], classes[-1]]
    utts = [(n, list(lab)) for L in range(4) for lab in itertools.product(classes, repeat=L) for n in GRID_T]
    for call, b in enumerate(range(0, len(utts), 31)):
        part = utts[b:b + 31]
        part.insert((7 * call + 3) % (len(part) + 1), (0, []))
        yield [n for n, _ in part], [lab for _, lab in part]


def gpu_mmi(y, lens, labels, den, lam=0.0, window=None, totals=None, nan_padding=False, ws_bytes=None):
    """y [T, S, K] CPU float32 -> dict of numpy outputs; window (pad, off): both matrices are column windows of wider ones"""
    T, S, K = y.shape
    y = y.clone() if isinstance(y, torch.Tensor) else torch.from_numpy(np.array(y))
    if nan_padding:
        for s, n in enumerate(lens):
            y[max(n, 0):, s] = float("nan")
    if window:
        pad, off = window
        yw = torch.full((T * S, K + pad), 7.0, device="cuda")
        yw[:, off:off + K] = y.reshape(T * S, K).cuda()
        yd = yw[:, off:off + K]
        dw = torch.full((T * S, K + 2 * pad), 5.0, device="cuda")
        dd = dw[:, off:off + K]
    else:
        yd, dd = y.reshape(T * S, K).cuda().contiguous(), torch.full((T * S, K), 5.0, device="cuda")
    if ws_bytes is None:
        r = k.ctc_mmi_eval(yd, lens, labels, den, ctc_weight=lam, diff=dd, totals=totals)
    else:
        r = raw_eval(yd, lens, labels, den, lam, dd, ws_bytes, totals)
    torch.cuda.synchronize()
    out = dict(loss=r.loss.cpu().numpy(), diff=r.diff.cpu().numpy().reshape(T, S, K), num_logp=r.num_logp.cpu().numpy(),
               den_logz=r.den_logz.cpu().numpy(), lm_logw=r.lm_logw.cpu().numpy())
    if window:
        dw[:, off:off + K] = 5.0
        assert bool((dw == 5.0).all()), "columns outside the window were touched"
    return out


def raw_eval(yd, lens, labels, den, lam, dd, ws_bytes, totals=None):
    """the C entry with a workspace of ws_bytes: the label capacity, and with it the reference chain's plan, follows from the size"""
    S = len(lens)
    T, K = yd.shape[0] // S, yd.shape[1]
    lens_dev = torch.tensor(lens, dtype=torch.int32, device="cuda")
    lab, off, _ = k.ctc.pack_labels(labels, yd.device)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    o = [torch.empty(S, device="cuda") for _ in range(4)]
    st = load_library().klstm_ctc_mmi_eval(yd.data_ptr(), T, S, K, yd.stride(0), lens_dev.data_ptr(), lab.data_ptr(), off.data_ptr(), den.blank,
                                           den.graph.data_ptr(), ctypes.c_size_t(den.graph_bytes), den.states, float(lam), dd.data_ptr(),
                                           dd.stride(0), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(),
                                           totals.data_ptr() if totals is not None else None, ws.data_ptr(), ctypes.c_size_t(ws_bytes), None)
    assert st == 0, load_library().klstm_last_error()
    return k.CtcMmiResult(o[0], dd, o[1], o[2], o[3])


def check_call(y, lens, labels, lm, den, blank, lam, tag, window=None, nan_padding=False):
    """one call against truth64 under the bar, with the identities that need no tolerance choice; returns the device's outputs"""
    y = y if isinstance(y, torch.Tensor) else torch.from_numpy(y)
    T, S, K = y.shape
    t64 = M.truth64(y.numpy(), lens, labels, lm, blank, lam)
    l32, d32 = M.plain32(y.numpy(), lens, labels, lm, blank, lam, status=t64["status"])
    e32, r32 = M.pooled_errors(l32, d32, t64, lens)
    g = gpu_mmi(y, lens, labels, den, lam, window=window, nan_padding=nan_padding)
    e, r = M.pooled_errors(g["loss"], g["diff"], t64, lens)
    bar_e, bar_r = max(4 * e32, FLOOR), max(4 * r32, FLOOR)
    print(f"{tag}: diff {e:.3g} (plain32 {e32:.3g}) loss {r:.3g} (plain32 {r32:.3g})", flush=True)
    for s, n in enumerate(lens):
        st = t64["status"][s]
        if st == "counted":
            assert np.isfinite(g["loss"][s]) and g["loss"][s] >= -bar_r * max(1.0, abs(t64["loss"][s])), (tag, s, g["loss"][s])
            assert not g["diff"][n:, s].any(), (tag, s, "padding rows")
            if lam == 0.0:
                assert np.abs(g["diff"][:n, s].astype(np.float64).sum(-1)).max() <= K * 2.0 ** -23, (tag, s, "rows sum to 0")
            assert abs(g["num_logp"][s] - t64["num_logp"][s]) <= 1e-5 * max(1.0, abs(t64["num_logp"][s]))
            assert abs(g["lm_logw"][s] - t64["logw"][s]) <= 1e-6 * max(1.0, abs(t64["logw"][s]))
        else:
            assert not g["diff"][:, s].any(), (tag, s, st)
            assert g["loss"][s] == (np.inf if st == "rejected" else 0.0), (tag, s, st, g["loss"][s])
            assert g["num_logp"][s] == 0 and g["den_logz"][s] == 0 and g["lm_logw"][s] == 0
    bound(e, bar_e, f"{tag} diff")
    bound(r, bar_r, f"{tag} loss")
    return g, t64


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K,blank,lms,window", GRID, ids=[f"K{g[0]}b{g[1]}" for g in GRID])
def test_grid(K, blank, lms, window, kind):
    gen = torch.Generator().manual_seed(11 * K + blank)
    counted = rejected = 0
    for name in lms:
        lm, den = device_lm(name, K, blank)
        for c, (lens, labels) in enumerate(grid_calls(K, blank)):
            y = R.small_posteriors(kind, 9, len(lens), K, gen)
            lam = (0.0, 0.3)[c % 2]
            _, t64 = check_call(y, lens, labels, lm, den, blank, lam, f"{name} {kind} call {c}", window=window if c % 2 == 0 else None,
                                nan_padding=c % 3 == 0)
            counted += t64["status"].count("counted")
            rejected += t64["status"].count("rejected")
    assert counted > 20 and rejected > 5


def random_labels(rng, K, blank, n):
    classes = [c for c in range(K) if c != blank]
    return [classes[i] for i in rng.randint(0, len(classes), n)]


@pytest.mark.parametrize("name,K", [("bigram", 24), ("trigram", 8)])
def test_more_than_one_pass_per_thread(name, K):
    """Q K = 600 / 584 table cells: the arc pass of the beta chain takes several arcs per thread"""
    blank, T = 0, 40
    lm, den = device_lm(name, K, blank)
    rng = np.random.RandomState(K)
    lens = [40, 33, 0, 17]
    labels = [random_labels(rng, K, blank, n) for n in (9, 6, 0, 5)]
    for kind in ("flat", "peaked"):
        y = R.small_posteriors(kind, T, 4, K, torch.Generator().manual_seed(K))
        check_call(y, lens, labels, lm, den, blank, 0.2, f"{name} K {K} {kind}")


@functools.lru_cache(maxsize=None)
def cap_case():
    """Q K = 16384, the capacity: a random dense automaton, half of its arcs absent (weight 0, next -1 or beyond Q)"""
    Q = K = 128
    rng = np.random.RandomState(5)
    nxt = rng.randint(0, Q, (Q, K)).astype(np.int32)
    w = rng.uniform(0.2, 1.5, (Q, K)).astype(np.float32)
    kill = rng.randint(0, 6, (Q, K))
    w[kill == 0] = 0
    nxt[kill == 1] = -1
    nxt[kill == 2] = Q + 3
    fin = rng.uniform(0, 1, Q).astype(np.float32)
    fin[rng.randint(0, 3, Q) == 0] = 0
    lm = (nxt, w, fin)
    labels, pres = [], M.present(lm, 0)
    for seed in (1, 2):                          # two references the automaton accepts: walks along present arcs to a final state
        r2, q, lab = np.random.RandomState(seed), 0, []
        while len(lab) < 2 or fin[q] <= 0:
            ok = [c for c in range(1, K) if pres[q, c] and (not lab or c != lab[-1])]
            c = ok[r2.randint(len(ok))]
            lab.append(c)
            q = int(nxt[q, c])
        labels.append(lab)
    return lm, labels


def test_capacity_cap():
    lm, labels = cap_case()
    den = k.CtcMmiDenominator(k.CtcLabelLm(*lm), blank=0)
    assert max(len(l) for l in labels) <= 8, labels
    T, K = 8, 128
    y = R.small_posteriors("flat", T, 2, K, torch.Generator().manual_seed(3))
    _, t64 = check_call(y, [8, 8], labels, lm, den, 0, 0.0, "capacity")
    assert t64["status"] == ["counted", "counted"]


@functools.lru_cache(maxsize=None)
def plan_case():
    K, blank, T = 5, 0, 9
    lm, den = device_lm("bigram", K, blank)
    rng = np.random.RandomState(9)
    lens = [9, 5, 0, 9, 7, 2]
    labels = [random_labels(rng, K, blank, n) for n in (3, 2, 0, 4, 1, 5)]
    y = R.small_posteriors("flat", T, len(lens), K, torch.Generator().manual_seed(4))
    return lm, den, y, lens, labels


def test_every_plan_of_the_reference_chain_gives_the_same_bytes():
    """label capacities 3 / 100 / 200 / 400 / 1023 select the five chain geometries of klstm_ctc_eval; the denominator has one plan"""
    lm, den, y, lens, labels = plan_case()
    T, S, K = y.shape
    base = None
    for cap in (5, 100, 200, 400, 1023):
        g = gpu_mmi(y, lens, labels, den, 0.3, ws_bytes=k.ctc_mmi_workspace_bytes(T, S, K, den.states, cap))
        if base is None:
            base = g
            t64 = M.truth64(y.numpy(), lens, labels, lm, 0, 0.3)
            assert t64["status"].count("counted") >= 3
        for key in base:
            assert base[key].tobytes() == g[key].tobytes(), (cap, key)
    # a capacity below a stream's labels rejects that stream and leaves the others alone
    g = gpu_mmi(y, lens, labels, den, 0.3, ws_bytes=k.ctc_mmi_workspace_bytes(T, S, K, den.states, 3))
    assert g["loss"][3] == np.inf and g["loss"][0] == base["loss"][0]


@pytest.mark.parametrize("kind", ["peaked", "nearflat"])
def test_rescaling_over_300_frames(kind):
    """T = 300, K = 48: an unscaled float32 alpha (about 48^-300 on flat rows) would underflow many times over"""
    K, blank, T = 48, 0, 300
    lm, den = device_lm("bigram", K, blank)
    rng = np.random.RandomState(48)
    lens = [300, 0, 150, 77]
    labels = [random_labels(rng, K, blank, n) for n in (40, 0, 25, 10)]
    gen = torch.Generator().manual_seed(6)
    y = torch.softmax(torch.randn(T, 4, K, generator=gen) * (8.0 if kind == "peaked" else 0.05), -1)
    g, t64 = check_call(y, lens, labels, lm, den, blank, 0.0, f"rescaling {kind}")
    assert t64["status"] == ["counted", "idle", "counted", "counted"] and (t64["logz"][[0, 2, 3]] < -1).all()


def test_all_ones_lm_reproduces_ctc_eval():
    K, blank, T = 7, 2, 9
    lm = M.all_ones_lm(K)
    den = k.CtcMmiDenominator(k.CtcLabelLm(*lm), blank=blank)
    rng = np.random.RandomState(2)
    lens = [9, 4, 0, 9, 2, 6]
    labels = [random_labels(rng, K, blank, n) for n in (3, 2, 0, 0, 4, 1)]
    for kind in KINDS:
        y = R.small_posteriors(kind, T, len(lens), K, torch.Generator().manual_seed(8))
        yd = y.reshape(-1, K).cuda()
        ul, d = k.ctc_eval(yd, lens, labels, blank=blank)
        g = gpu_mmi(y, lens, labels, den, 0.5)
        ul, d = ul.cpu().numpy(), d.cpu().numpy().reshape(T, -1, K)
        t64 = M.truth64(y.numpy(), lens, labels, lm, blank, 0.5)
        l32, d32 = M.plain32(y.numpy(), lens, labels, lm, blank, 0.5, status=t64["status"])
        e32, r32 = M.pooled_errors(l32, d32, t64, lens)
        for s, st in enumerate(t64["status"]):
            if st != "counted":
                assert g["loss"][s] == ul[s]
                continue
            assert (-g["num_logp"][s]).tobytes() == ul[s].tobytes(), (kind, s)
            assert abs(g["loss"][s] - ul[s]) <= max(4 * r32, FLOOR) * max(1.0, abs(ul[s])) + 9 * 2.0 ** -23     # (log Z: nine float32 row sums)
            assert np.abs(g["diff"][:, s] - 1.5 * d[:, s]).max() <= max(4 * e32, FLOOR) + 1.5 * 2.0 ** -22


def test_reproducible_and_independent_of_the_stream():
    lm, den, y, lens, labels = plan_case()
    T, S, K = y.shape
    tot = torch.zeros(5, dtype=torch.float64, device="cuda")
    a = gpu_mmi(y, lens, labels, den, 0.3, totals=tot)
    b = gpu_mmi(y, lens, labels, den, 0.3, totals=tot)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key
    perm = [4, 2, 5, 0, 3, 1]
    c = gpu_mmi(y[:, perm], [lens[p] for p in perm], [labels[p] for p in perm], den, 0.3)
    for key in a:
        want = a[key][:, perm] if key == "diff" else a[key][perm]
        assert np.ascontiguousarray(want).tobytes() == c[key].tobytes(), key
    t64 = M.truth64(y.numpy(), lens, labels, lm, 0, 0.3)
    ls = cnt = rej = fr = nl = 0.0
    for s, st in enumerate(t64["status"]):
        if st == "counted":
            ls += float(a["loss"][s]); cnt += 1; fr += lens[s]; nl += float(-a["num_logp"][s])
        elif st == "rejected":
            rej += 1
    assert tot.cpu().tolist() == [2 * ls, 2 * cnt, 2 * rej, 2 * fr, 2 * nl] and rej >= 1 and cnt >= 3


def test_error_paths():
    lib = load_library()
    lm, den, y, lens, labels = plan_case()
    T, S, K = y.shape
    Q = den.states
    yd, dd = y.reshape(-1, K).cuda(), torch.empty(T * S, K, device="cuda")
    lens_dev = torch.tensor(lens, dtype=torch.int32, device="cuda")
    lab, off, _ = k.ctc.pack_labels(labels, yd.device)
    nbytes = k.ctc_mmi_workspace_bytes(T, S, K, Q, 8)
    ws = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
    loss = torch.empty(S, device="cuda")
    other = k.CtcMmiDenominator(k.CtcLabelLm(*lm), blank=1)

    def call(**kw):
        a = dict(y=yd.data_ptr(), T=T, S=S, K=K, stride=K, lens=lens_dev.data_ptr(), lab=lab.data_ptr(), off=off.data_ptr(), blank=0,
                 graph=den.graph.data_ptr(), gbytes=ctypes.c_size_t(den.graph_bytes), Q=Q, lam=0.0, diff=dd.data_ptr(), dstride=K,
                 loss=loss.data_ptr(), nl=None, lz=None, lw=None, tot=None, ws=ws.data_ptr(), nbytes=ctypes.c_size_t(nbytes), st=None)
        a.update(kw)
        return lib.klstm_ctc_mmi_eval(*a.values()), lib.klstm_last_error()
    assert call()[0] == 0
    arg = [dict(y=None), dict(lens=None), dict(lab=None), dict(off=None), dict(graph=None), dict(diff=None), dict(loss=None), dict(ws=None),
           dict(T=0), dict(Q=0), dict(blank=K), dict(blank=-1), dict(stride=K - 1), dict(dstride=K - 1), dict(diff=yd.data_ptr()),
           dict(lam=-1.0), dict(lam=float("nan")), dict(ws=ws.data_ptr() + 4), dict(graph=den.graph.data_ptr() + 4),
           dict(nbytes=ctypes.c_size_t(k.ctc_mmi_workspace_bytes(T, S, K, Q, 0) - 1)), dict(gbytes=ctypes.c_size_t(den.graph_bytes - 1)),
           dict(graph=den.graph.data_ptr() + 256),                                  # nothing was built there
           dict(blank=1),                                                           # built for blank 0
           dict(graph=other.graph.data_ptr(), gbytes=ctypes.c_size_t(other.graph_bytes)),      # built for blank 1
           dict(Q=Q - 1)]                                                           # built for Q states
    for kw in arg:
        st, msg = call(**kw)
        assert st == 1 and msg.startswith(b"klstm_ctc_mmi_eval"), (kw, st, msg)
    for kw in [dict(S=33), dict(T=65536 // S + 1), dict(Q=16384 // K + 1), dict(K=1)]:
        st, msg = call(**kw)
        assert st == 2 and msg.startswith(b"klstm_ctc_mmi_eval"), (kw, st, msg)

    dlm = k.CtcLabelLm(*lm)
    gbuf = torch.empty(den.graph_bytes + 16, dtype=torch.uint8, device="cuda")

    def build(**kw):
        a = dict(Q=Q, K=K, blank=0, nxt=dlm.next.data_ptr(), w=dlm.weight.data_ptr(), fin=dlm.final.data_ptr(), g=gbuf.data_ptr(),
                 gbytes=ctypes.c_size_t(den.graph_bytes), st=None)
        a.update(kw)
        return lib.klstm_ctc_mmi_graph_build(*a.values()), lib.klstm_last_error()
    assert build()[0] == 0 and build(fin=None)[0] == 0
    for kw in [dict(nxt=None), dict(w=None), dict(g=None), dict(Q=0), dict(blank=K), dict(g=gbuf.data_ptr() + 4),
               dict(gbytes=ctypes.c_size_t(den.graph_bytes - 1))]:
        st, msg = build(**kw)
        assert st == 1 and msg.startswith(b"klstm_ctc_mmi_graph_build"), (kw, st, msg)
    for kw in [dict(Q=16384 // K + 1), dict(K=1)]:
        st, msg = build(**kw)
        assert st == 2 and msg.startswith(b"klstm_ctc_mmi_graph_build"), (kw, st, msg)
    with pytest.raises(k.KlstmError) as ei:
        k.ctc_mmi_workspace_bytes(T, S, K, Q, 1024)
    assert ei.value.status == 2
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end through the C++ classes (include/klstm_nnet.hpp CtcMmi, TrainMmiWholeUtterances; tests/cpp/ctc_mmi_test.cpp)
# ---------------------------------------------------------------------------------------------------------------------------------
# the CTC epochs of tests/test_ctc_mbr_gpu.py's schedule per kind of net, and the MMI learning rate (half the CTC one)
SCHEDULE = {"blstm": (20, 0.005), "lstm": (50, 0.005)}


@pytest.mark.parametrize("kind", ["blstm", "lstm"])
def test_cpp_trainer_lowers_the_mmi_loss(kind, tmp_path):
    from tests.test_ctc_mmi import run_driver
    dump = str(tmp_path / "dump.bin")
    epochs, lr = SCHEDULE[kind]
    r = run_driver("train", kind, dump, epochs, lr)
    kv = dict(f.split("=") for f in r.stdout.split() if "=" in f)
    print(f"ctc_mmi_test train {kind}:", r.stdout.strip(), flush=True)
    assert float(kv["loss_after"]) < float(kv["loss_before"]), (kv["loss_before"], kv["loss_after"])
    assert float(kv["loss_after"]) >= 0
    # 12 training utterances and the one the bigram rejects are handed out, the 120-frame one is skipped by the batcher
    assert int(kv["done"]) == 13 and int(kv["skipped"]) == 1 and int(kv["rejected"]) == 1
    # the minibatch the driver dumped (its second: the objects had been through another shape): Python's path gives the same bits
    raw = np.fromfile(dump, dtype=np.int32)
    T, S, K, Q, nlab = (int(v) for v in raw[:5])
    p = 5

    def take(n, dtype=np.int32):
        nonlocal p
        a = raw[p:p + n].view(dtype)
        p += n
        return a
    lens, off, flat = take(S).tolist(), take(S + 1).tolist(), take(nlab).tolist()
    nxt, w, fin = take(Q * K).reshape(Q, K), take(Q * K, np.float32).reshape(Q, K), take(Q, np.float32)
    post, diff, loss = take(T * S * K, np.float32).reshape(T * S, K), take(T * S * K, np.float32), take(S, np.float32)
    assert p == raw.size
    refs = [flat[off[s]:off[s + 1]] for s in range(S)]
    den = k.CtcMmiDenominator(k.CtcLabelLm(nxt.copy(), w.copy(), fin.copy()), blank=0)
    mine = k.ctc_mmi_eval(torch.from_numpy(post.copy()).cuda(), lens, refs, den, ctc_weight=0.1)
    assert mine.diff.cpu().numpy().tobytes() == diff.tobytes() and mine.loss.cpu().numpy().tobytes() == loss.tobytes()
    assert diff.any() and np.isfinite(loss).any()
