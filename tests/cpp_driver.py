"""The stand-alone C++ drivers under tests/cpp/ that the host-side tests build against libklstm.so and run: one build() and one run()
behind the build_*_driver() / run_driver() of every test file that has one."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ("klstm.h", "klstm_component.hpp", "klstm_kaldi_io.hpp", "klstm_trainer.hpp", "klstm_nnet.hpp", "klstm_blstm.hpp")


def build(name, headers=HEADERS, flags=("-O1",)):
    """tests/cpp/<name>.cpp -> tests/cpp/<name>, again whenever the source or one of the include/ headers listed is newer"""
    import kaldi_lstm_amd as k
    lib, exe = k.lib_path(), os.path.join(ROOT, "tests", "cpp", name)
    assert os.path.exists(lib), "libklstm.so missing: run __graft_entry__.build()"
    deps = [exe + ".cpp"] + [os.path.join(ROOT, "include", h) for h in headers]
    if (not os.path.exists(exe)) or any(os.path.getmtime(f) > os.path.getmtime(exe) for f in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", *flags, "-I" + os.path.join(ROOT, "include"), exe + ".cpp",
                               "-L" + os.path.dirname(lib), "-lklstm", "-Wl,-rpath,$ORIGIN/../../kaldi-lstm_amd", "-o", exe])
    return exe


def run(name, *args, ok=True, timeout=900, headers=HEADERS):
    """the driver's completed process; ok: it must have ended with status 0 and an output that begins with OK"""
    r = subprocess.run([build(name, headers)] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    if ok:
        assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    return r
