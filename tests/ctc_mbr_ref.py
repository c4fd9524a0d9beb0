"""Yardsticks of the n-best risk tests (tests/test_ctc_mbr.py, tests/test_ctc_mbr_gpu.py; klstm_ctc_mbr_eval of include/klstm.h), host only:
  parts()      per stream and labelling, by torch.nn.functional.ctc_loss on the CPU: l_q = -loss and gamma_q = softmax - grad, in
               float64 (the truth) or float32 ("stock fp32": losses, gamma and weights all in float32 -- the yardstick of the bars)
  compose()    P = softmax(kappa l), R = sum P W, diff = kappa sum_q P_q (W_q - R) gamma_q + lambda (y - gamma_ref) from such parts
  oracle()     the two in one call
  statuses()   which entries are dropped and which streams are idle / rejected / skipped, from lengths and labels alone
  random_refs(), peaked(), make_case()  seeded PEAKED posteriors (a bump per reference label at its proportional frame) with the n-best lists and edit distances
               of tests/ctc_beam_ref.beam_twin
The small suite (tests/test_ctc_mbr_small.py, tests/test_ctc_mbr_small_gpu.py) has yardsticks of its own, which take the RAW posteriors
as the kernel does (clamped at FLT_MIN, rows not renormalised) and know dropped entries and stream statuses:
  objective64()   one stream in float64 numpy from the log-domain forward-backward of tests/ctc_ref.truth_core
  truth64()       objective64 over the counted streams of a call with the dropped entries taken out (statuses())
  twin32()        the recipe documented in include/klstm.h in numpy float32 / double, on ctc_ref.norm_twin -- never the kernel
  enumerate_objective()   risk, posterior and diff from ALL K^n frame paths, no forward-backward: pins objective64
  small_list(), small_group(), complete_case()   the lists and the calls of the small suite, computed once"""
import functools
import itertools

import numpy as np
import torch
import torch.nn.functional as F

from tests import ctc_beam_ref as B
from tests import ctc_ref as R
from tests.ctc_ref import FLT_MIN, infeasible


def statuses(lens, lists, costs, counts, refs, K, blank, T, N, max_len, lam, stride=None):
    """-> (stream status [S]: 'idle' | 'rejected' | 'skipped' | 'counted', dropped [S][count] bools).  lists[s][q]: the labels of entry
    q; costs[s][q]; counts[s]: the listed entries; refs: S label lists (looked at when lam > 0)"""
    status, dropped = [], []
    for s, n in enumerate(lens):
        cnt = counts[s]
        drop = []
        if 0 <= cnt <= N:
            for q in range(cnt):
                lab = list(lists[s][q])
                too_long = len(lab) > max_len or (stride is not None and len(lab) > stride)
                drop.append(bool(too_long or infeasible([max(n, 1)], [lab], K, blank)[0]))
        dropped.append(drop)
        if n == 0:
            status.append("idle")
        elif n < 0 or n > T or cnt < 0 or cnt > N or (lam > 0 and (len(refs[s]) > max_len or infeasible([n], [refs[s]], K, blank)[0])):
            status.append("rejected")
        elif cnt == 0 or any(costs[s][q] < 0 for q in range(cnt)) or all(drop):
            status.append("skipped")
        else:
            status.append("counted")
    return status, dropped


def _one(a_log, n, lab, blank):
    """(loss, gamma [n, K]) of one labelling on one stream; a_log [n, K] log posteriors of the wanted dtype"""
    a = a_log.clone().requires_grad_()
    sm = F.log_softmax(a, -1)
    loss = F.ctc_loss(sm[:, None], torch.tensor([list(lab)], dtype=torch.long).reshape(1, -1), torch.tensor([n]), torch.tensor([len(lab)]),
                      blank=blank, reduction="none", zero_infinity=True)[0]
    loss.backward()
    return loss.detach(), torch.exp(sm.detach()) - a.grad


def parts(y, lens, lists, refs, blank, dtype=torch.float64, streams=None):
    """y [T, S, K] float32.  -> per stream None (not in `streams`) or dict(logp [n_q], gamma [n_q][n, K], ref_loss, ref_gamma, ysm): the
    log probability and the occupation of every entry of lists[s], and of refs[s] where refs is given; tensors of `dtype`"""
    y = torch.as_tensor(y, dtype=torch.float32)
    out = []
    for s in range(y.shape[1]):
        if streams is not None and s not in streams:
            out.append(None)
            continue
        n = lens[s]
        a = torch.log(torch.clamp_min(y[:n, s], FLT_MIN)).to(dtype)
        lg = [_one(a, n, lab, blank) for lab in lists[s]]
        d = dict(logp=[-l for l, _ in lg], gamma=[g for _, g in lg], ysm=torch.softmax(a, -1), ref_loss=None, ref_gamma=None)
        if refs is not None:
            l, g = _one(a, n, refs[s], blank)
            d["ref_loss"], d["ref_gamma"] = l, g
        out.append(d)
    return out


def compose(pt, costs, kappa, lam, T, K):
    """-> dict(risk [S] float64, diff [T, S, K] float64, post [S] lists, logp [S] lists, ref_loss [S]) from parts(); everything is
    computed in the dtype of the parts and only then widened"""
    S = len(pt)
    risk, diff = np.zeros(S), np.zeros((T, S, K))
    post, logp, ref_loss = [[] for _ in range(S)], [[] for _ in range(S)], np.zeros(S)
    for s, d in enumerate(pt):
        if d is None or not d["logp"]:
            continue
        dt = d["logp"][0].dtype
        l = torch.stack(d["logp"])
        P = torch.softmax(torch.tensor(kappa, dtype=dt) * l, 0)
        W = torch.tensor([float(c) for c in costs[s]], dtype=dt)
        R = (P * W).sum()
        c = P * (W - R)
        n = d["gamma"][0].shape[0]
        g = torch.zeros(n, K, dtype=dt)
        for q in range(len(c)):
            g = g + torch.tensor(kappa, dtype=dt) * c[q] * d["gamma"][q]
        if lam > 0:
            g = g + torch.tensor(lam, dtype=dt) * (d["ysm"] - d["ref_gamma"])
            ref_loss[s] = float(d["ref_loss"])
        risk[s] = float(R)
        diff[:n, s] = g.double().numpy()
        post[s] = [float(v) for v in P]
        logp[s] = [float(v) for v in l]
    return dict(risk=risk, diff=diff, post=post, logp=logp, ref_loss=ref_loss)


def oracle(y, lens, lists, costs, refs, blank, kappa, lam, dtype=torch.float64):
    """every stream counted, every entry feasible (statuses() says which are).  refs may be None when lam == 0"""
    T, _, K = np.asarray(y).shape
    return compose(parts(y, lens, lists, refs if lam > 0 else None, blank, dtype), costs, kappa, lam, T, K)


def random_refs(seed, K, ref_lens, blank=0, no_repeats=False):
    """seeded label sequences without the blank; no_repeats: no two adjacent labels equal (a labelling as long as half its frames)"""
    g = torch.Generator().manual_seed(seed)
    refs = []
    for L in ref_lens:
        lab = torch.randint(0, K - 1, (L,), generator=g)
        lab = (lab + (lab >= blank).long()).tolist()
        if no_repeats:
            for j in range(1, L):
                while lab[j] == lab[j - 1] or lab[j] == blank:
                    lab[j] = (lab[j] + 1) % K
        refs.append(lab)
    return refs


def peaked(seed, T, K, lens, refs, blank=0, sigma=0.5, bump=4.0):
    """y [T, S, K] float32 torch: logits = sigma * randn, + bump on the class of reference label j at frame floor((j + 0.5) n / L),
    + 0.6 bump on the blank of every frame; posteriors = their softmax"""
    g = torch.Generator().manual_seed(seed + 7919)
    z = torch.randn(T, len(lens), K, generator=g) * sigma
    z[:, :, blank] += 0.6 * bump
    for s, lab in enumerate(refs):
        for j, c in enumerate(lab):
            z[int((j + 0.5) * lens[s] / len(lab)), s, c] += bump
    return torch.softmax(z, -1)


def make_case(seed, T, K, lens, ref_lens, blank=0, sigma=0.5, bump=4.0, beam=16, cands=8, nbest=8):
    """-> dict(y [T, S, K] float32 torch, refs, lists [S][count] label lists, costs [S][count], counts [S]): peaked() posteriors around
    random_refs(), the lists and edit distances that the beam search's twin finds on them"""
    S = len(lens)
    refs = random_refs(seed, K, ref_lens, blank)
    y = peaked(seed, T, K, lens, refs, blank, sigma, bump)
    tw = B.beam_twin(y.numpy(), lens, blank, beam, cands, nbest, refs=refs)
    counts = [int(c) for c in tw["nbest_count"]]
    lists = [[list(h) for h in tw["hyp"][s][:counts[s]]] for s in range(S)]
    costs = [[int(e) for e in tw["errors"][s][:counts[s]]] for s in range(S)]
    return dict(y=y, refs=refs, lists=lists, costs=costs, counts=counts)


# ---------------------------------------------------------------------------------------------------------------------------------
# the small suite: raw posteriors, float64 truth, the documented recipe in float32, path enumeration
# ---------------------------------------------------------------------------------------------------------------------------------
def objective64(y, lists, costs, ref, blank, kappa, lam):
    """One stream.  y [n, K] FLOAT64 posteriors taken as given: raw, rows not renormalised, emissions log(max(y, FLT_MIN)) as
    ctc_ref.truth64 takes them; lists: the LIVE entries (all feasible), costs theirs; ref: the reference labels (read when lam > 0).
    l_q and gamma_q from ctc_ref.truth_core; P = softmax(kappa l), R = sum P W, diff = kappa sum_q P_q (W_q - R) gamma_q +
    lam (y - gamma_ref), all in float64 numpy.  -> dict(risk, diff [n, K], logp [n_q], post [n_q], ref_loss)"""
    y = np.asarray(y, dtype=np.float64)
    fb = [R.truth_core(y, list(lab), blank) for lab in lists]
    l = np.array([lp for lp, _ in fb], dtype=np.float64)
    W = np.asarray(costs, dtype=np.float64)
    z = kappa * l
    P = np.exp(z - z.max())
    P = P / P.sum()
    risk = float((P * W).sum())
    diff = np.zeros_like(y)
    for q, (_, gam) in enumerate(fb):
        diff += kappa * P[q] * (W[q] - risk) * gam
    ref_loss = 0.0
    if lam > 0:
        lp, gam = R.truth_core(y, list(ref), blank)
        diff += lam * (y - gam)
        ref_loss = float(-lp)
    return dict(risk=risk, diff=diff, logp=l, post=P, ref_loss=ref_loss)


def _as_float(v):
    """risk_scale and ctc_weight reach the kernel as C floats: both yardsticks take the value the kernel is given"""
    return float(np.float32(v))


def _live(y, lens, lists, costs, counts, refs, blank, kappa, lam, N, max_len, hyp_stride):
    y = torch.as_tensor(y, dtype=torch.float32).numpy()
    T, S, K = y.shape
    status, dropped = statuses(lens, lists, costs, counts, refs, K, blank, T, N, max_len, lam, stride=hyp_stride)
    live = [[q for q in range(counts[s]) if not dropped[s][q]] if status[s] == "counted" else [] for s in range(S)]
    out = dict(risk=np.zeros(S), diff=np.zeros((T, S, K)), post=[[] for _ in range(S)], logp=[[] for _ in range(S)],
               ref_loss=np.zeros(S), status=status, dropped=dropped, live=live)
    return y, out


def truth64(y, lens, lists, costs, counts, refs, blank, kappa, lam, N, max_len, hyp_stride):
    """One call.  y [T, S, K] float32; lists[s][q], costs[s][q], counts[s], refs[s] as statuses() takes them.  objective64 over the
    counted streams with the dropped entries removed, on double(y); zeros elsewhere.  -> compose()'s dict (post and logp hold the LIVE
    entries in order) and status [S], dropped [S][count], live [S] (the indices of the live entries)"""
    kappa, lam = _as_float(kappa), _as_float(lam)
    y, out = _live(y, lens, lists, costs, counts, refs, blank, kappa, lam, N, max_len, hyp_stride)
    for s, live in enumerate(out["live"]):
        if not live:
            continue
        n = lens[s]
        o = objective64(y[:n, s].astype(np.float64), [lists[s][q] for q in live], [costs[s][q] for q in live],
                        refs[s] if lam > 0 else None, blank, kappa, lam)
        out["risk"][s], out["diff"][:n, s], out["ref_loss"][s] = o["risk"], o["diff"], o["ref_loss"]
        out["post"][s], out["logp"][s] = [float(v) for v in o["post"]], [float(v) for v in o["logp"]]
    return out


def twin32(y, lens, lists, costs, counts, refs, blank, kappa, lam, N, max_len, hyp_stride):
    """The arguments and the result of truth64().  The recipe include/klstm.h documents, never the kernel: per live entry l_q (the double
    ctc_ref.norm_twin returns, negated) and gamma_q = y - diff_q in float32; P and R in double, q ascending; the coefficient
    kappa P_q (W_q - R) rounded to float once; the row accumulated in float32, q ascending, the reference last with the coefficient
    -lam, and added to lam * y.  diff comes back as float32, risk / post / logp / ref_loss as the float32 values the kernel stores"""
    kappa, lam = _as_float(kappa), _as_float(lam)
    y, out = _live(y, lens, lists, costs, counts, refs, blank, kappa, lam, N, max_len, hyp_stride)
    out["diff"] = out["diff"].astype(np.float32)
    lam32 = np.float32(lam)
    for s, live in enumerate(out["live"]):
        if not live:
            continue
        n = lens[s]
        ys = y[:n, s]
        tw = [R.norm_twin(ys, list(lists[s][q]), blank) for q in live]
        l = [-loss for loss, _ in tw]
        W = [float(costs[s][q]) for q in live]
        m = max(kappa * v for v in l)
        wexp = [float(np.exp(kappa * v - m)) for v in l]
        Z = 0.0
        for w in wexp:
            Z += w
        inv = 1.0 / Z
        risk = 0.0
        for w, c in zip(wexp, W):
            risk += w * inv * c
        acc = np.zeros_like(ys)
        for w, c, (_, d) in zip(wexp, W, tw):
            coef = np.float32(kappa * (w * inv * (c - risk)))
            acc = acc + coef * (ys - d)
        if lam > 0:
            loss, d = R.norm_twin(ys, list(refs[s]), blank)
            acc = acc + (-lam32) * (ys - d)
            acc = lam32 * ys + acc
            out["ref_loss"][s] = float(np.float32(loss))
        out["risk"][s], out["diff"][:n, s] = float(np.float32(risk)), acc
        out["post"][s] = [float(np.float32(w * inv)) for w in wexp]
        out["logp"][s] = [float(np.float32(v)) for v in l]
    return out


def enumerate_objective(y, lists, costs, blank, kappa):
    """Brute force over all K^n frame paths for a list that is COMPLETE, i.e. holds every labelling of non-zero probability; y [n, K]
    float64 taken as given (clamp it first where it has zeros), no forward-backward.  The paths are collapsed as ctc_mmi_ref.enumerate_z
    collapses them and pooled per labelling: p_q = sum of its paths, occ_q(t, k) = sum of its paths through class k at frame t.  Then
    P_q = p_q^kappa / sum, R = sum_q P_q W_q, diff = kappa sum_q P_q (W_q - R) occ_q / p_q -- at kappa = 1 that is
    R = sum_paths p(path) W(collapse) / sum_paths p(path) and diff(t, k) = sum_paths P(path) (W - R) [path_t = k].
    -> dict(risk, diff [n, K], post [n_q], logp [n_q], total: the sum over ALL paths, missing: the mass of the paths whose labelling
    is not in the list -- exactly 0.0 for a complete list)"""
    y = np.asarray(y, dtype=np.float64)
    n, K = y.shape
    index = {tuple(lab): q for q, lab in enumerate(lists)}
    assert len(index) == len(lists), "an entry is listed twice"
    p, occ = np.zeros(len(lists)), np.zeros((len(lists), n, K))
    total = missing = 0.0
    rows = np.arange(n)
    for path in itertools.product(range(K), repeat=n):
        col = tuple(k for k in (k for k, _ in itertools.groupby(path)) if k != blank)
        pr = float(np.prod(y[rows, list(path)]))
        total += pr
        q = index.get(col)
        if q is None:
            missing += pr
            continue
        p[q] += pr
        occ[q, rows, list(path)] += pr
    W = np.asarray(costs, dtype=np.float64)
    logp = np.log(p)
    z = kappa * logp
    P = np.exp(z - z.max())
    P = P / P.sum()
    risk = float((P * W).sum())
    diff = np.zeros((n, K))
    for q in range(len(lists)):
        diff += kappa * P[q] * (W[q] - risk) * occ[q] / p[q]
    return dict(risk=risk, diff=diff, post=P, logp=logp, total=total, missing=missing)


def small_list(K, blank):
    """the list every stream of the small suite carries: every labelling of length 0, 1, 2 over the non-blank classes c0 < c1 < ... in
    itertools.product order; at K = 4 also [c0,c0,c0], [c0,c1,c0], [c2,c1,c0] (N = 16, the limit of list_n); at K = 2 also [c0,c0,c0]
    (N = 4); N = 7 at K = 3"""
    c = [v for v in range(K) if v != blank]
    out = [list(lab) for L in range(3) for lab in itertools.product(c, repeat=L)]
    if K == 4:
        out += [[c[0], c[0], c[0]], [c[0], c[1], c[0]], [c[2], c[1], c[0]]]
    if K == 2:
        out += [[c[0], c[0], c[0]]]
    return out


SMALL_SCALES = [(1.0, 0.0), (0.5, 0.3), (4.0, 0.0), (0.05, 0.3)]     # (risk_scale, ctc_weight) the calls of a group cycle through
SMALL_MAX_LEN, SMALL_STRIDE = 31, 3


def small_scales(K, blank):
    """(kappa, lam) of every call of ctc_ref.small_grid(K, blank): SMALL_SCALES in order, call 0 taking the first pair -- except that a
    group with fewer calls than the cycle has pairs (K = 2: two calls, the second of five streams) begins at the second pair, so that
    its full call runs with the reference in use: a reference can be rejected only where lam > 0, and all six infeasible references
    of K = 2 sit in call 0"""
    n = sum(1 for _ in R.small_grid(K, blank))
    first = 1 if n < len(SMALL_SCALES) else 0
    return [SMALL_SCALES[(first + i) % len(SMALL_SCALES)] for i in range(n)]


def small_call(y, lens, refs, K, blank, kappa, lam):
    """one call of the small suite from posteriors, lengths and references: every stream lists small_list(K, blank) with the edit
    distances to its reference; truth64 and twin32 at (kappa, lam)"""
    entries = small_list(K, blank)
    N, S = len(entries), len(lens)
    lists = [[list(e) for e in entries] for _ in range(S)]
    costs = [[int(B.levenshtein(e, refs[s])) for e in entries] for s in range(S)]
    counts = [N] * S
    args = (y, lens, lists, costs, counts, refs, blank, kappa, lam, N, SMALL_MAX_LEN, SMALL_STRIDE)
    return dict(y=y, lens=lens, refs=refs, lists=lists, costs=costs, counts=counts, N=N, K=K, blank=blank, kappa=_as_float(kappa),
                lam=_as_float(lam), t64=truth64(*args), tw=twin32(*args))


@functools.lru_cache(maxsize=None)
def small_group(K, blank, kind, seed=7):
    """the calls of one (K, blank, kind) group: ctc_ref.small_grid's lengths, its labels as the REFERENCES, ctc_ref.small_posteriors in
    the order and with the seed of ctc_ref.small_group, (kappa, lam) from small_scales(); one small_call() dict each.  Computed once
    per session and shared: nothing may modify it"""
    g = torch.Generator().manual_seed(seed)
    calls = []
    for (lens, labels), (kappa, lam) in zip(R.small_grid(K, blank), small_scales(K, blank)):
        y = R.small_posteriors(kind, R.SMALL_T, len(lens), K, g)
        calls.append(small_call(y, lens, labels, K, blank, kappa, lam))
    return calls


def pooled(out, t64, lens, wmax_of=None):
    """(max |diff - truth| over the valid rows, max |risk - truth|, max |logp - truth| / max(1, |truth|) over the live entries, the
    largest live cost) pooled over the counted streams of a call; out: a twin32() dict, or the device's outputs in its layout"""
    e = r = l = 0.0
    wmax = 0
    for s, live in enumerate(t64["live"]):
        if t64["status"][s] != "counted":
            continue
        n = lens[s]
        e = max(e, float(np.abs(np.asarray(out["diff"][:n, s], dtype=np.float64) - t64["diff"][:n, s]).max()))
        r = max(r, abs(float(out["risk"][s]) - t64["risk"][s]))
        want = np.array(t64["logp"][s])
        l = max(l, float((np.abs(np.array(out["logp"][s], dtype=np.float64) - want) / np.maximum(1.0, np.abs(want))).max()))
        if wmax_of is not None:
            wmax = max(wmax, max(wmax_of[s][q] for q in live))
    return e, r, l, wmax


def feasible_labellings(K, blank, n):
    """every labelling with an alignment to n frames, shortest first, in itertools.product order"""
    c = [v for v in range(K) if v != blank]
    labs = [list(lab) for L in range(n + 1) for lab in itertools.product(c, repeat=L)]
    return [lab for lab in labs if not infeasible([n], [lab], K, blank)[0]]


COMPLETE_T = {3: 4, 2: 5}           # K -> the longest stream whose complete list fits list_n = 16 (15 labellings at T = 4, K = 3)


@functools.lru_cache(maxsize=None)
def complete_case(K, blank, kind, seed=11):
    """One call whose stream s has s + 1 frames and lists EVERY labelling feasible at that length (K = 3: 3, 5, 9, 15 entries at
    T = 1..4; K = 2: 1 + ceil(T / 2) at T = 1..5), so that at kappa = 1 P is the true posterior over labellings.  Costs: the edit
    distance to [c0, c1] (K = 3) or [c0] (K = 2); lam = 0.  -> a small_call()-like dict with N = 16 and hyp_stride = T, plus enum [S]:
    enumerate_objective of every stream on max(double(y), FLT_MIN)"""
    T = COMPLETE_T[K]
    c = [v for v in range(K) if v != blank]
    ref = c[:2] if K == 3 else c[:1]
    lens = list(range(1, T + 1))
    g = torch.Generator().manual_seed(seed + 10 * K + blank)
    y = R.small_posteriors(kind, T, T, K, g)
    lists = [feasible_labellings(K, blank, n) for n in lens]
    costs = [[int(B.levenshtein(e, ref)) for e in l] for l in lists]
    counts = [len(l) for l in lists]
    refs = [list(ref) for _ in lens]
    args = (y, lens, lists, costs, counts, refs, blank, 1.0, 0.0, 16, SMALL_MAX_LEN, T)
    yd = np.maximum(y.numpy().astype(np.float64), FLT_MIN)
    enum = [enumerate_objective(yd[:n, s], lists[s], costs[s], blank, 1.0) for s, n in enumerate(lens)]
    return dict(y=y, lens=lens, refs=refs, lists=lists, costs=costs, counts=counts, N=16, K=K, blank=blank, kappa=1.0, lam=0.0,
                t64=truth64(*args), tw=twin32(*args), enum=enum, yd=yd)
