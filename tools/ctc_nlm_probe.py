"""What the neural second pass costs: device time per call of CtcNeuralLm.rescore (per group of E entries and chunk of T positions
knlm_pack -> propagate_inference per layer -> affine_propagate -> knlm_score_rows, then one knlm_rank) next to the ctc_beam_decode call
that produced the lists, to the n-gram second pass (ctc_nbest_rescore with an order-5 token model), and to the same scores obtained with
the calls the library had before: host-made one-hot rows uploaded per chunk, the same engines and Affine, klstm_log_softmax_scatter in
SCORE_LOGPOST into a full rows x V matrix, a torch gather and an index_add in double (the composition; its host plan is built outside
the timed region).  The lists are those of tools/ctc_rescore_probe.py (K = 32, about 100 and 300 tokens per entry, N = 8 and 64, S = 1 and
32; at 300 tokens N = 8 only: the composition uploads 5 MB of one-hot rows per chunk).  LMs: one and two layers of 800 cells / 512
projections, at V = 32 (one-hot input) and V = 4096 (an embedding of 512 rows, the 32 tokens its first classes), E = 16, T = 20.  The plan is laid out for max_len = the lists' stride (the frames of the search), since the
lengths are not read back: the share of rows that carry no position is recorded.  Device events around warmed-up repeats that end in a
synchronise, the legs alternating, TRIALS times; the median and the spread are kept.  Writes profiles/ctc_nlm_probe.json (DESIGN.md 4u
quotes it).

With --stages: where a chunk goes on the first shape, stage by stage, and the whole call with a stream of its own and with
"persist_verify" off (profiles/ctc_nlm_stages.json; see stages()).

    python tools/ctc_nlm_probe.py [--iters 3] [--warmup 1] [--out profiles/ctc_nlm_probe.json] [--quick] [--stages]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import kaldi_lstm_amd as k  # noqa: E402
from tools.ctc_probe import timed  # noqa: E402
from tools.ctc_rescore_probe import K, batch, language  # noqa: E402

C, R, D, E, T, TRIALS = 800, 512, 512, 16, 20, 3


def make_lm(V, n_lstm, seed=3):
    rng = np.random.RandomState(seed)
    cols = V if V <= 64 else D

    def u(*shape, scale=0.05):
        return ((rng.rand(*shape) - 0.5) * 2 * scale).astype(np.float32)
    layers = []
    for l in range(n_lstm):
        i = cols if l == 0 else R
        layers.append((u(4 * C * i + 4 * C * R + 4 * C + 3 * C + R * C), i, C, R))
    embed = None if V <= 64 else (u(D, V, scale=0.5), u(D))
    return dict(layers=layers, W=u(V, R, scale=0.2), b=u(V), embed=embed, V=V)


def host_plan(nb, max_len):
    """what the composition needs on the host: per (group, chunk) the input class of every row (-1: a zero row), and on the device the
    target, the mask and the entry of every row.  Built once per shape, outside the timed region: it reads the lists back"""
    hyp, n, cnt = nb.hyp.cpu().numpy(), nb.hyp_len.cpu().numpy(), nb.nbest_count.cpu().numpy()
    S, N, _ = hyp.shape
    chunks = (max_len + 1 + T - 1) // T
    groups = (S * N + E - 1) // E
    X = np.full((groups * E, chunks * T), -1, np.int64)
    TG = np.zeros((groups * E, chunks * T), np.int64)
    for se in range(S * N):
        if se % N >= cnt[se // N]:
            continue
        toks = hyp[se // N, se % N, :n[se // N, se % N]]
        X[se, 0], X[se, 1:len(toks) + 1], TG[se, :len(toks)] = 0, toks, toks
    # [group][chunk][t][e]
    x = X.reshape(groups, E, chunks, T).transpose(0, 2, 3, 1).reshape(groups * chunks, T * E)
    tg = TG.reshape(groups, E, chunks, T).transpose(0, 2, 3, 1).reshape(groups * chunks, T * E)
    ent = np.minimum(np.arange(groups)[:, None, None] * E + np.arange(E)[None, None, :] + np.zeros((1, chunks * T, 1), np.int64), S * N - 1)
    return dict(SN=S * N, chunks=chunks, x=np.ascontiguousarray(x), tg=torch.from_numpy(np.ascontiguousarray(tg)).cuda(),
                mask=torch.from_numpy(np.ascontiguousarray(x >= 0)).cuda(), ent=torch.from_numpy(ent.reshape(groups * chunks, T * E)).cuda(),
                rows=groups * chunks * T * E, real_rows=int((x >= 0).sum()))


class Composition:
    """the same scores with the calls the library had before the knlm_* entries"""

    def __init__(self, lm, dev_lm, plan):
        self.m, self.V, self.p = dev_lm, lm["V"], plan
        self.host = np.zeros((T * E, self.V), np.float32)
        self.onehot = torch.empty(T * E, self.V, device="cuda")
        self.logpost = torch.empty(T * E, self.V, device="cuda")
        self.dst = torch.arange(T * E, dtype=torch.int32, device="cuda")

    def __call__(self):
        m, p = self.m, self.p
        acc = torch.zeros(p["SN"], dtype=torch.float64, device="cuda")
        for i in range(p["x"].shape[0]):
            if i % p["chunks"] == 0:
                for e in m.engines:
                    e.reset(np.ones(E, np.int32))
            x = p["x"][i]
            on = x >= 0
            self.host[:] = 0
            self.host[np.nonzero(on)[0], x[on]] = 1
            self.onehot.copy_(torch.from_numpy(self.host))
            h = self.onehot
            if m.embed is not None:
                k.affine_propagate(h, m.embed[0], m.embed[1], m.x)
                h = m.x
            for l, e in enumerate(m.engines):
                e.propagate_inference(h, m.h[l])
                h = m.h[l]
            k.affine_propagate(h, m.W, m.b, m.a)
            k.log_softmax_scatter(m.a, self.dst, self.logpost, k.SCORE_LOGPOST)
            lp = self.logpost.gather(1, p["tg"][i][:, None])[:, 0].double() * p["mask"][i]
            acc.index_add_(0, p["ent"][i], lp)
        return acc


def stages(a, lang):
    """--stages: where a chunk goes, on the first shape (S = 1, N = 8, 300 frames).  Per LM: every stage of the chunk loop alone and
    in combinations (microseconds per chunk, 16 chunks a call), the whole call with the default streams, with a stream of its own
    (CtcNeuralLm(stream=...)) and with "persist_verify" off, next to the composition; the engines' counters.  Writes
    profiles/ctc_nlm_stages.json"""
    y, lens, refs = batch(lang["sents"], 1, 100)
    nb = k.ctc_beam_decode(y, lens, beam=16, cands=8, nbest=8, refs=k.ctc.pack_labels(refs, y.device), lm=lang["bigram"])
    max_len = min(1023, nb.hyp.shape[2])
    chunks = (max_len + 1 + T - 1) // T
    lists = (nb.hyp, nb.hyp_len, nb.nbest_count, None)
    plan = host_plan(nb, max_len)
    out = {}
    for V in (32, 4096):
        for n in (1, 2):
            name, lm = "%dx%d_V%d" % (n, C, V), make_lm(V, n)
            kw = dict(embed=lm["embed"], bos=0, eos=0, num_stream=E, chunk=T, classes=K)
            m = k.CtcNeuralLm(lm["layers"], lm["W"], lm["b"], **kw)
            own = k.CtcNeuralLm(lm["layers"], lm["W"], lm["b"], stream=torch.cuda.Stream(), **kw)
            comp = Composition(lm, m, plan)
            acc = torch.zeros(8, dtype=torch.float64, device="cuda")
            pos = torch.zeros(8, dtype=torch.int32, device="cuda")

            def stage(which):
                for c in range(chunks):
                    if "pack" in which:
                        k.knlm_pack(lists, K, V, 0, 0, 0, E, T, c * T, m.x, m.embed, nb.score, max_len)
                    h = m.x
                    for l, e in enumerate(m.engines):
                        if "lstm%d" % l in which:
                            e.propagate_inference(h, m.h[l])
                        h = m.h[l]
                    if "affine" in which:
                        k.affine_propagate(h, m.W, m.b, m.a)
                    if "score" in which:
                        k.knlm_score_rows(m.a, lists, K, 0, 0, E, T, c * T, acc, pos, nb.score, max_len, m.ws)
            lstms = tuple("lstm%d" % l for l in range(n))
            r = {"chunks": chunks, "us_per_chunk": {}}
            for w in (("pack",),) + tuple((l,) for l in lstms) + (("affine",), ("score",), lstms, ("pack",) + lstms, lstms + ("affine",),
                                                                     ("pack",) + lstms + ("affine", "score")):
                r["us_per_chunk"]["+".join(w)] = round(statistics.median(timed(lambda: stage(w), a.iters, a.warmup) for _ in range(TRIALS)) / chunks, 1)
            legs = {"fused_default_streams_us": lambda: m.rescore(nb, nlm_scale=0.5), "fused_own_stream_us": lambda: own.rescore(nb, nlm_scale=0.5),
                    "composition_us": comp}
            times = {nm: [] for nm in legs}
            for _ in range(TRIALS):
                for nm, leg in legs.items():
                    times[nm].append(timed(leg, a.iters, a.warmup))
            for nm, v in times.items():
                r[nm] = round(statistics.median(v), 1)
                r[nm + "_min_max"] = [round(min(v), 1), round(max(v), 1)]
            r["max_abs_difference_own_stream"] = float((own.accumulate(nb)[0] - m.accumulate(nb)[0]).abs().max())
            r["persist_giveups"] = [e.profile_query("persist_giveups")[1] for e in m.engines]
            r["fwd_inference_launches"] = [e.profile_query("fwd_inference_launches")[1] for e in m.engines]
            for e in m.engines:
                e.set_option("persist_verify", 0)
            r["fused_default_streams_persist_verify_0_us"] = round(statistics.median(timed(legs["fused_default_streams_us"], a.iters, a.warmup)
                                                                                       for _ in range(TRIALS)), 1)
            out[name] = r
            print(name, json.dumps(r), flush=True)
            m.close()
            own.close()
    path = a.out if a.out.endswith("stages.json") else os.path.join(os.path.dirname(a.out), "ctc_nlm_stages.json")
    with open(path, "w") as fh:
        json.dump({"what": "S = 1, N = 8, 300 frames, about 100 tokens per entry; device microseconds, medians of %d trials of %d calls; "
                           "us_per_chunk: the named stages of the chunk loop alone, per chunk" % (TRIALS, a.iters), "lms": out}, fh, indent=1)
        fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--quick", action="store_true", help="the smallest shape only")
    ap.add_argument("--stages", action="store_true", help="the stage-by-stage record of the first shape instead (profiles/ctc_nlm_stages.json)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_nlm_probe.json"))
    a = ap.parse_args()
    lang = language()
    if a.stages:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        return stages(a, lang)
    lms = {"%dx%d_V%d" % (n, C, V): make_lm(V, n) for V in (32, 4096) for n in (1, 2)}
    dev = {name: k.CtcNeuralLm(lm["layers"], lm["W"], lm["b"], embed=lm["embed"], bos=0, eos=0, num_stream=E, chunk=T, classes=K)
           for name, lm in lms.items()}
    rows = []
    shapes = [(100, 1, 8)] if a.quick else [(100, 1, 8), (100, 1, 64), (100, 32, 8), (100, 32, 64), (300, 1, 8), (300, 32, 8)]
    for L, S, N in shapes:
        y, lens, refs = batch(lang["sents"], S, L)
        packed = k.ctc.pack_labels(refs, y.device)
        beam = max(16, N)

        def search():
            return k.ctc_beam_decode(y, lens, beam=beam, cands=8, nbest=N, refs=packed, lm=lang["bigram"])
        nb = search()
        max_len = min(1023, nb.hyp.shape[2])
        r = {"S": S, "T_frames": 3 * L, "K": K, "N": N, "E": E, "T": T, "max_len": max_len, "entries_listed": int(nb.nbest_count.sum()),
             "tokens_per_entry": round(float(nb.hyp_len.sum()) / max(1, int(nb.nbest_count.sum())), 1)}
        legs = {"beam_us": (search, 10), "rescore_order5_us": (lambda: k.ctc_nbest_rescore(nb, add=lang["order5"], sub=lang["bigram"]), 10)}
        comps, plan = {}, host_plan(nb, max_len)
        for name, m in dev.items():
            comps[name] = Composition(lms[name], m, plan)
            legs["nlm_%s_us" % name] = ((lambda m=m: m.rescore(nb, nlm_scale=0.5)), a.iters)
            legs["composition_%s_us" % name] = (comps[name], a.iters)
        r["rows_per_call"], r["padding_row_share"] = plan["rows"], round(1.0 - plan["real_rows"] / plan["rows"], 4)
        for name, m in dev.items():                                  # the two paths score the same thing
            fused, comp = m.accumulate(nb)[0].view(-1), comps[name]()
            r["max_abs_difference_%s" % name] = float((fused - comp).abs().max())
        times = {name: [] for name in legs}
        for _ in range(TRIALS):
            for name, (leg, iters) in legs.items():
                times[name].append(timed(leg, iters, a.warmup))
        for name, v in times.items():
            r[name] = round(statistics.median(v), 1)
            r[name + "_min_max"] = [round(min(v), 1), round(max(v), 1)]
        for name in dev:
            r["fused_over_composition_%s" % name] = round(r["nlm_%s_us" % name] / r["composition_%s_us" % name], 3)
        rows.append(r)
        print(json.dumps(r), flush=True)
    out = {"what": "device microseconds per call through the Python entries, median of %d trials (%d calls each for the neural legs, 10 for the "
                   "search and the n-gram pass); K = 32; LMs of %d cells / %d projections, %d streams, chunks of %d positions; V = 4096 with an "
                   "embedding of %d rows" % (TRIALS, a.iters, C, R, E, T, D),
           "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
