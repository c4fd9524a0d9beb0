"""CPU checks of the C-ABI library: it loads without a GPU, exports every symbol that
include/klstm.h declares, and refuses (loudly) to create an engine when no device exists."""
import os
import re
import subprocess

import pytest
import torch

from tests import cpp_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    txt = open(os.path.join(ROOT, "include", "klstm.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(klstm_[a-z_0-9]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    import kaldi_lstm_amd as k
    lib = k.load_library()
    names = declared_symbols()
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), f"libklstm.so does not export {n}"
    assert b"gfx950" in lib.klstm_version()


def test_exported_names_are_the_recorded_list():
    """the klstm_* names the library defines are those of tests/golden/klstm_abi_names.txt: whichever translation unit an entry lives in"""
    import kaldi_lstm_amd as k
    out = subprocess.run(["nm", "-D", "--defined-only", k.lib_path()], capture_output=True, text=True, check=True).stdout
    have = sorted({ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("klstm_")})
    want = open(os.path.join(ROOT, "tests", "golden", "klstm_abi_names.txt")).read().split()
    assert len(want) == 100 and want == sorted(want)
    assert have == want, f"lost {sorted(set(want) - set(have))}, added {sorted(set(have) - set(want))}"


def test_one_error_string_behind_the_entries_of_three_translation_units():
    """tests/cpp/error_channel_test.cpp: an entry of klstm_engine.hip, one of klstm_api_ctc.hip and one of klstm_api_ops.hip fail their
    argument checks (before any HIP call: no GPU needed) and klstm_last_error() reads each message; a second thread reads an empty string
    meanwhile: the string is one thread_local of the library, not one per translation unit"""
    cpp_driver.build("error_channel_test", headers=("klstm.h",), flags=("-O1", "-pthread"))
    cpp_driver.run("error_channel_test", headers=("klstm.h",))


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_cpu_fallback():
    import kaldi_lstm_amd as k
    with pytest.raises(k.KlstmError) as ei:
        k.Engine(40, 800, 512, 4)
    assert ei.value.status == 5          # KLSTM_ERR_NOGPU
    assert "no CPU fallback" in str(ei.value)


def test_product_package_never_touches_the_oracle():
    pkg = os.path.join(ROOT, "kaldi-lstm_amd")
    for dp, _, fns in os.walk(pkg):
        for fn in fns:
            if fn.endswith((".py", ".hip", ".h", ".hpp", ".cpp")):
                src = open(os.path.join(dp, fn), errors="ignore").read()
                assert not re.search(r"import\s+oracle|from\s+oracle|#include[^\n]*oracle|liblstmp_oracle|lstmp_oracle_",
                                     src), f"{fn} references the oracle"


def test_every_kernel_launch_goes_through_the_one_helper():
    """launch() in csrc/klstm_kernels.h is the only code that launches a kernel or raises a kernel's dynamic-LDS limit: one probe
    branch, one error convention, and the limit raised once per (device, kernel) under its lock."""
    csrc = os.path.join(ROOT, "kaldi-lstm_amd", "csrc")
    for fn in sorted(os.listdir(csrc)):
        if not fn.endswith((".hip", ".h")):
            continue
        src = open(os.path.join(csrc, fn)).read()
        src = re.sub(r"//[^\n]*|/\*.*?\*/", "", src, flags=re.S)
        if fn == "klstm_kernels.h":
            a, b = src.index("inline hipError_t raise_lds_limit("), src.index("hipError_t launch(K kern")
            b = src.index("\n}\n", b)
            src = src[:a] + src[b:]
        for name in ("hipFuncSetAttribute", "hipLaunchKernelGGL", "hipExtLaunchKernelGGL", "<<<"):
            assert name not in src, f"{fn} calls {name} outside launch() (klstm_kernels.h)"
