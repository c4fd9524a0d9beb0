"""What the CTC forced alignment costs: device time of klstm_ctc_align next to klstm_ctc_eval on the same posteriors at the 24 shapes of
tools/ctc_probe.py (S = 8 / 16 / 32 streams, T = 500 / 1000 frames, L = 50 / 150 labels, K = 64 / 4096 classes), next to the host route
(net_out.cpu() + the numpy twin of tests/ctc_align_ref.py, wall clock, once), and the call's two parts -- the chain alone, the trace
alone -- at T = 500 / 1000 / 2000 / 8000.  Device events around 10 warmed-up calls that end in a synchronise, the fastest of three
alternating rounds, all legs in one process on one tensor.  Prints one JSON line per measurement and tables at the end (DESIGN.md 4j
records them; profiles/ctc_align_probe.txt).

The parts need a build of the library that can run them alone: klstm_ctc_align.hip compiled with -DKLSTM_ALIGN_PROBE (nothing else
differs; the other objects are those of the package's own build), linked into tools/libklstm_align_probe.so and loaded in place of the
package's library:

    python tools/ctc_align_probe.py --build        (needs hipcc and the package's object files: where the package was built)
    python tools/ctc_align_probe.py [--iters 10] [--warmup 3] [--no-host]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_LIB = os.path.join(ROOT, "tools", "libklstm_align_probe.so")
sys.path.insert(0, ROOT)


def build_probe_library():
    import importlib.util
    spec = importlib.util.spec_from_file_location("klstm_build", os.path.join(ROOT, "kaldi-lstm_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = os.path.join(ROOT, "build_probe")
    os.makedirs(objdir, exist_ok=True)
    src = "csrc/klstm_ctc_align.hip"
    obj = os.path.join(objdir, "klstm_ctc_align.hip.o")
    subprocess.check_call([hipcc] + b.FLAGS + ["-DKLSTM_ALIGN_PROBE", "-c", os.path.join(b.HERE, src), "-o", obj])
    objs = [obj if s == src else os.path.join(b.OBJDIR, os.path.basename(s) + ".o") for s in b.SRCS]
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", PROBE_LIB] + objs + ["-ldl"])
    return PROBE_LIB


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--build", action="store_true")
    a = ap.parse_args()
    if a.build:
        print(build_probe_library())
        return
    assert os.path.exists(PROBE_LIB), "run tools/ctc_align_probe.py --build where the package was built"
    os.environ["KLSTM_LIB_PATH"] = PROBE_LIB
    import numpy as np
    import torch
    import kaldi_lstm_amd as k
    from tests import ctc_align_ref as A

    def timed(step):
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters

    def fastest(legs):
        """legs: dict name -> step; three alternating rounds, the fastest of each leg, device microseconds per call"""
        best = {n: float("inf") for n in legs}
        for _ in range(3):
            for n, step in legs.items():
                best[n] = min(best[n], timed(step))
        return {n: round(v, 1) for n, v in best.items()}

    def case(S, T, L, K):
        g = torch.Generator(device="cuda").manual_seed(S * 7 + T + L + K)
        lens = [T - (37 * s) % (T // 4) for s in range(S)]
        labs = [max(1, L - (5 * s) % (L // 2)) for s in range(S)]
        labs[0] = L
        y = torch.softmax(torch.randn(T * S, K, generator=g, device="cuda") * 4.0, -1)
        labels = [(torch.randint(1, K, (n,), generator=g, device="cuda")).tolist() for n in labs]
        return y, lens, labels, k.ctc.pack_labels(labels, y.device), torch.tensor(lens, dtype=torch.int32, device="cuda")

    def phases(v):
        os.environ["KLSTM_ALIGN_PHASES"] = str(v)

    def align_step(y, ld, packed, ph=3):
        def step():
            phases(ph)
            k.ctc_align(y, ld, packed, 0)
        return step

    rows = []
    for S in (8, 16, 32):
        for T in (500, 1000):
            for K in (64, 4096):
                for L in (50, 150):
                    y, lens, labels, packed, ld = case(S, T, L, K)
                    diff = torch.empty_like(y)
                    t = fastest({"align": align_step(y, ld, packed), "ctc_eval": lambda: k.ctc_eval(y, ld, packed, 0, diff)})
                    res = k.ctc_align(y, ld, packed, 0)
                    assert bool(torch.isfinite(res.score).all())
                    r = {"S": S, "T": T, "L": L, "K": K, "align_us": t["align"], "ctc_eval_us": t["ctc_eval"],
                         "align_over_ctc_eval": round(t["align"] / t["ctc_eval"], 3)}
                    if not a.no_host:
                        torch.cuda.synchronize()
                        w0 = time.perf_counter()
                        yh = y.cpu().numpy().reshape(T, S, K)
                        w1 = time.perf_counter()
                        tw = A.align_twin(yh, lens, labels, 0, dtype=np.float32)
                        w2 = time.perf_counter()
                        fc = res.frame_class.cpu().numpy().reshape(T, S)
                        r.update(host_copy_us=round((w1 - w0) * 1e6, 1), host_twin_us=round((w2 - w1) * 1e6, 1),
                                 host_over_align=round((w2 - w0) * 1e6 / t["align"], 1),
                                 frames_off_the_fp32_twin=int(sum((fc[:n, s] != tw[s]["frame_class"][:n]).sum() for s, n in enumerate(lens))))
                    rows.append(r)
                    print(json.dumps(r), flush=True)
    parts = []
    for T in (500, 1000, 2000, 8000):
        for L in (50, 150):
            y, lens, labels, packed, ld = case(8, T, L, 64)
            k.ctc_align(y, ld, packed, 0)                            # the pointers the trace-only leg walks
            t = fastest({"call": align_step(y, ld, packed, 3), "chain": align_step(y, ld, packed, 1), "trace": align_step(y, ld, packed, 2)})
            phases(3)
            r = {"S": 8, "T": T, "L": L, "K": 64, "call_us": t["call"], "chain_only_us": t["chain"], "trace_only_us": t["trace"],
                 "trace_share_of_call_pct": round(100.0 * t["trace"] / t["call"], 1)}
            parts.append(r)
            print(json.dumps(r), flush=True)
    print("\n  S     T    L     K  align us  ctc_eval us  ratio" + ("" if a.no_host else "    host us  host/align"))
    for r in rows:
        print(f"{r['S']:3d} {r['T']:5d} {r['L']:4d} {r['K']:5d} {r['align_us']:9.1f} {r['ctc_eval_us']:12.1f} {r['align_over_ctc_eval']:6.3f}" +
              ("" if a.no_host else f" {r['host_copy_us'] + r['host_twin_us']:10.0f} {r['host_over_align']:11.1f}"))
    print("\n  S     T    L   call us  chain us  trace us  trace share")
    for r in parts:
        print(f"{r['S']:3d} {r['T']:5d} {r['L']:4d} {r['call_us']:9.1f} {r['chain_only_us']:9.1f} {r['trace_only_us']:9.1f} {r['trace_share_of_call_pct']:10.1f}%")


if __name__ == "__main__":
    main()
