"""krnnt_band_eval_bf16 without a GPU (include/klstm_rnnt.h, THE BF16 JOINT): the refusals it shares with krnnt_band_eval under its own
name, all before the first HIP call, and the workspace: the banded formula plus the stated bf16 copies of W."""
import ctypes

import pytest


@pytest.mark.parametrize("kw,status", [(dict(S=33), 2), (dict(R=65), 2), (dict(J=24), 2), (dict(V=4097), 2), (dict(blank=5), 2),
                                       (dict(enc=None), 1), (dict(band=None), 1), (dict(es=15), 1), (dict(bg=None), 1), (dict(short=1), 1)],
                         ids=str)
def test_refusals_carry_the_entrys_name(kw, status):
    import kaldi_lstm_amd as k
    lib = k.load_library()
    p = ctypes.c_void_p(256)                            # never dereferenced: refused before any pointer is followed
    a = dict(T=4, S=1, Umax=2, J=16, V=5, blank=0, R=2, enc=p, band=p, es=16, bg=p, short=-(1 << 40))
    a.update(kw)
    nbytes = ctypes.c_size_t(lib.krnnt_band_bf16_workspace_bytes(4, 1, 2, 2, 16, 5, 1) - a["short"])
    got = lib.krnnt_band_eval_bf16(a["enc"], a["es"], p, 16, p, p, a["T"], a["S"], a["Umax"], a["J"], a["V"], p, p, p, a["blank"], a["R"],
                                   a["band"], p, 16, p, 16, p, a["bg"], p, None, p, nbytes, None)
    assert got == status and lib.klstm_last_error().startswith(b"krnnt_band_eval_bf16:")


def test_workspace_is_the_banded_one_plus_the_copies_of_w():
    import kaldi_lstm_amd as k
    lib = k.load_library()
    up, up32 = lambda v: (v + 255) // 256 * 256, lambda v: (v + 31) // 32 * 32
    T, S, Umax, R, J, V = 33, 3, 16, 9, 48, 130
    wb, wbt = up(2 * V * up32(J)), up(2 * J * up32(V))
    assert lib.krnnt_band_bf16_workspace_bytes(T, S, Umax, R, J, V, 1) == lib.krnnt_band_workspace_bytes(T, S, Umax, R, J, V) + wb + wbt
    assert lib.krnnt_band_bf16_workspace_bytes(T, S, Umax, R, J, V, 0) == lib.krnnt_band_forward_workspace_bytes(T, S, R) + wb
    assert k.rnnt_band_workspace_bytes(T, S, Umax, R, J, V, precision="bf16") == k.rnnt_band_workspace_bytes(T, S, Umax, R, J, V) + wb + wbt
    assert lib.krnnt_band_bf16_workspace_bytes(T, S, 1024, R, J, V, 1) == 0 and lib.klstm_last_error().startswith(b"krnnt_band_bf16_workspace_bytes:")
    assert lib.krnnt_band_bf16_workspace_bytes(T, S, Umax, 65, J, V, 0) == 0
    for call in (lambda: k.rnnt_band_workspace_bytes(T, S, Umax, R, J, V, precision="int8"),
                 lambda: k.rnnt_band_eval(None, None, None, None, None, None, None, R, precision="int8")):
        with pytest.raises(ValueError):
            call()
