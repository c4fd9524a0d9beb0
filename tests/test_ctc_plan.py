"""The host helpers of the CTC lattice losses (csrc/klstm_ctc_host.h: ctc_chain_plan, ctc_chain_dispatch, ctc_label_capacity_of), without
a device.

tests/cpp/ctc_plan_test.cpp is a stand-alone program over the header alone (plain C++, no HIP), built with -fsanitize=address,undefined
and run on the host: the plan table at both edges of every plan, the dispatcher's <NW, P> and its error, the bisection over a toy byte
count and over the loss's workspace formula, which the program computes for itself.  It prints that formula's byte counts;
klstm_ctc_workspace_bytes of the built library must answer the same, which pins the workspace of klstm_ctc_eval byte for byte.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "ctc_plan_test")
SRC = EXE + ".cpp"
HDR = os.path.join(ROOT, "kaldi-lstm_amd", "csrc", "klstm_ctc_host.h")


@pytest.fixture(scope="module")
def program_output():
    cxx = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    stale = (not os.path.exists(EXE)) or any(os.path.getmtime(f) > os.path.getmtime(EXE) for f in (SRC, HDR))
    if stale:
        tmp = EXE + ".tmp.%d" % os.getpid()
        subprocess.check_call([cxx, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", SRC, "-o", tmp])
        os.replace(tmp, EXE)
    res = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    return res.returncode, res.stdout


def test_standalone_program_under_address_and_undefined_sanitizers(program_output):
    code, out = program_output
    assert code == 0 and "all checks passed" in out, out


def test_the_library_answers_the_loss_formula_of_the_program(program_output):
    import kaldi_lstm_amd as k
    lib = k.load_library()
    points = [tuple(int(v) for v in line.split()[1:]) for line in program_output[1].splitlines() if line.startswith("loss_bytes ")]
    assert {p[:2] for p in points} == {(1, 1), (50, 32)} and {p[2] for p in points} >= {0, 1, 511, 1022, 1023}
    for T, S, L, want in points:
        assert lib.klstm_ctc_workspace_bytes(T, S, L) == want, (T, S, L)
    # (1, 1): a head of 256 bytes and two rows of four floats; (50, 32) at 1023 labels: 262144 bytes of head, 2 * 50 * 32 rows of 2048 floats
    assert (1, 1, 0, 256 + 32) in points and (50, 32, 1023, 262144 + 2 * 50 * 32 * 2048 * 4) in points
