"""Yardsticks of the n-best risk tests (tests/test_ctc_mbr.py, tests/test_ctc_mbr_gpu.py; klstm_ctc_mbr_eval of include/klstm.h), host only:
  parts()      per stream and labelling, by torch.nn.functional.ctc_loss on the CPU: l_q = -loss and gamma_q = softmax - grad, in
               float64 (the truth) or float32 ("stock fp32": losses, gamma and weights all in float32 -- the yardstick of the bars)
  compose()    P = softmax(kappa l), R = sum P W, diff = kappa sum_q P_q (W_q - R) gamma_q + lambda (y - gamma_ref) from such parts
  oracle()     the two in one call
  statuses()   which entries are dropped and which streams are idle / rejected / skipped, from lengths and labels alone
  random_refs(), peaked(), make_case()  seeded PEAKED posteriors (a bump per reference label at its proportional frame) with the n-best lists and edit distances
               of tests/ctc_beam_ref.beam_twin"""
import numpy as np
import torch
import torch.nn.functional as F

from tests import ctc_beam_ref as B
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
