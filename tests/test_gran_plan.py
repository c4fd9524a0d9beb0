"""The host's bookkeeping of the value-only granule rings (engine option "persist_gran"; csrc/klstm_kernels.h gran_plan), without a device.

Two checks: klstm_gran_plan (the exported pure function) driven from Python against a model of the two rings of a direction -- every slot a
launch polls must hold the poison pattern when the launch begins, whatever sequence of frame counts, growth and tagged launches came before
-- and tests/cpp/gran_plan_test.cpp, a stand-alone program over the same functions plus the state they move (gran_advance, gran_reset),
built with -fsanitize=address,undefined and run on the host.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "gran_plan_test")
SRC = EXE + ".cpp"
HDR = os.path.join(ROOT, "kaldi-lstm_amd", "csrc", "klstm_kernels.h")
CAP = 256


def _plan(lib, ordinal, T, last_other, slots, cap=0):
    out = (ctypes.c_int * 4)()
    lib.klstm_gran_plan.argtypes = [ctypes.c_uint, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.klstm_gran_plan.restype = None
    lib.klstm_gran_plan(ordinal, T, last_other, slots, cap, out)
    return dict(use=out[0], ring=out[1], npoison=out[2], grow_to=out[3])


class _Rings:
    """The two rings of one direction as flags (written since last poisoned), and the engine's record of them."""

    def __init__(self, lib, cap=0):
        self.lib, self.cap = lib, cap
        self.n, self.last, self.slots = 0, [0, 0], 0
        self.dirty = [np.zeros(0, bool), np.zeros(0, bool)]
        self.value = self.tagged = self.grows = 0

    def launch(self, T):
        cap = self.cap or CAP
        p = _plan(self.lib, self.n, T, self.last[1 - (self.n & 1)], self.slots, self.cap)
        if not p["use"]:
            assert T + 2 > cap
            self.tagged += 1
            return
        assert T + 2 <= cap
        if p["grow_to"]:
            assert T + 2 <= p["grow_to"] <= cap and p["grow_to"] > self.slots and (p["ring"], p["npoison"]) == (0, 0)
            self.slots = p["grow_to"]
            self.dirty = [np.zeros(self.slots, bool), np.zeros(self.slots, bool)]
            self.n, self.last = 0, [0, 0]
            self.grows += 1
        ring = p["ring"]
        assert ring == self.n & 1 and T + 2 <= self.slots and 0 <= p["npoison"] < self.slots
        assert not self.dirty[ring][1: T + 1].any(), f"launch {self.n} (T = {T}) would poll a slot that does not hold the poison pattern"
        self.dirty[ring][1: T + 1] = True
        self.dirty[1 - ring][1: p["npoison"] + 1] = False
        assert not self.dirty[1 - ring].any(), f"launch {self.n} (T = {T}) leaves the other ring dirty"
        self.last[ring], self.last[1 - ring] = T, 0
        self.n += 1
        self.value += 1


@pytest.fixture(scope="module")
def lib():
    import kaldi_lstm_amd as k
    return k.load_library()


@pytest.mark.parametrize("seq", [(20,) * 7, (8, 9) * 4, (20, 8, 20, 9, 8, 8, 30, 3, 3, 20), (3, 30, 3, 30, 3)])
def test_every_polled_slot_is_poisoned_over_sequences_of_frame_counts(lib, seq):
    r = _Rings(lib)
    for T in seq:
        r.launch(T)
    assert (r.value, r.tagged, r.grows, r.slots) == (len(seq), 0, 1, 32)


def test_rings_grow_with_the_frame_count_and_never_shrink(lib):
    r = _Rings(lib)
    for T in (20, 8, 40, 8, 40, 62, 63, 20, 254, 9, 254, 254, 20):
        r.launch(T)
    assert (r.grows, r.slots, r.tagged) == (4, 256, 0)


def test_above_the_cap_a_launch_keeps_the_tags_and_the_record_does_not_move(lib):
    r = _Rings(lib)
    for T in (20, 255, 20, 1000, 255, 9, 20, 255):
        r.launch(T)
    assert (r.tagged, r.value, r.n) == (4, 4, 4)
    r = _Rings(lib, cap=40)
    for T in (20, 38, 39, 38, 20, 39, 8):
        r.launch(T)
    assert (r.tagged, r.slots, r.grows) == (2, 40, 2)


def test_random_frame_counts(lib):
    rng = np.random.RandomState(1)
    r = _Rings(lib)
    for T in rng.randint(1, 300, size=2000):
        r.launch(int(T))
    assert r.value > 1200 and r.tagged > 100


def test_standalone_program_under_address_and_undefined_sanitizers():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    stale = (not os.path.exists(EXE)) or any(os.path.getmtime(f) > os.path.getmtime(EXE) for f in (SRC, HDR))
    if stale:
        tmp = EXE + ".tmp.%d" % os.getpid()
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                               "-Xarch_host", "-fno-sanitize-recover=undefined", SRC, "-o", tmp])
        os.replace(tmp, EXE)
    res = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert res.returncode == 0 and "all checks passed" in res.stdout, res.stdout
