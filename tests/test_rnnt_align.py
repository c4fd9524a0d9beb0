"""krnnt_align and krnnt_band_align without a GPU (include/klstm_rnnt.h, FORCED ALIGNMENT): the limits and argument checks, which all run
before the first HIP call, and the two workspace formulas of the header recomputed here."""
import ctypes

import pytest


def test_refused_shapes_and_arguments_without_a_gpu():
    import kaldi_lstm_amd as k
    lib = k.load_library()
    p = ctypes.c_void_p(256)                            # never dereferenced: refused before any pointer is followed
    big, odd = ctypes.c_size_t(1 << 40), ctypes.c_void_p(258)

    def full(T=4, S=1, Umax=2, J=16, V=5, blank=0, enc=p, es=16, lens=p, fr=p, lp=p, sc=p, ws=p, nbytes=big, **_):
        return lib.krnnt_align(enc, es, p, 16, p, p, T, S, Umax, J, V, lens, p, p, blank, fr, lp, sc, ws, nbytes, None)

    def band(T=4, S=1, Umax=2, J=16, V=5, blank=0, R=2, bf16=0, enc=p, es=16, lens=p, lo=p, fr=p, lp=p, sc=p, ws=p, nbytes=big):
        return lib.krnnt_band_align(enc, es, p, 16, p, p, T, S, Umax, J, V, lens, p, p, blank, R, lo, bf16, fr, lp, sc, ws, nbytes, None)

    shapes = [dict(S=0), dict(S=33), dict(T=0), dict(Umax=-1), dict(Umax=1024), dict(J=24), dict(J=1040), dict(V=1), dict(V=4097), dict(blank=5),
              dict(blank=-1)]
    for fn, name, cases in ((full, b"krnnt_align:", shapes + [dict(T=(1 << 14) + 1, Umax=1023)]),
                            (band, b"krnnt_band_align:", shapes + [dict(R=0), dict(R=65), dict(T=(1 << 18) + 1, R=64)])):
        for kw in cases:
            assert fn(**kw) == 2 and lib.klstm_last_error().startswith(name), (name, kw)        # KLSTM_ERR_SHAPE
        need = lib.krnnt_align_workspace_bytes(4, 1, 2) if fn is full else lib.krnnt_band_align_workspace_bytes(4, 1, 2, 16, 5, 0)
        args = [dict(enc=None), dict(lens=None), dict(fr=None), dict(sc=None), dict(ws=None), dict(es=15), dict(enc=odd), dict(fr=odd), dict(lp=odd),
                dict(sc=odd), dict(ws=ctypes.c_void_p(264)), dict(nbytes=ctypes.c_size_t(need - 1))] + ([] if fn is full else [dict(lo=None), dict(lo=odd)])
        for kw in args:
            assert fn(**kw) == 1 and lib.klstm_last_error().startswith(name), (name, kw)        # KLSTM_ERR_ARG
    wb = lib.krnnt_band_align_workspace_bytes(4, 1, 2, 16, 5, 1) - lib.krnnt_band_align_workspace_bytes(4, 1, 2, 16, 5, 0)
    assert band(bf16=1, nbytes=ctypes.c_size_t(need + wb - 1)) == 1 and wb == 512               # the bf16 copy of W counts
    assert lib.krnnt_align_workspace_bytes(4, 33, 2) == 0 and lib.klstm_last_error().startswith(b"krnnt_align_workspace_bytes:")
    assert lib.krnnt_band_align_workspace_bytes(4, 1, 65, 16, 5, 0) == 0 and lib.klstm_last_error().startswith(b"krnnt_band_align_workspace_bytes:")


def test_workspaces_are_the_documented_formulas():
    import kaldi_lstm_amd as k
    up = lambda v: (v + 255) // 256 * 256
    full = lambda T, S, Umax: up(16 * S) + 3 * up(4 * S * T * (Umax + 1)) + up(8 * S * (T + Umax + 1) * ((Umax + 64) // 64))
    band = lambda T, S, R, J, V, bf16: up(16 * S) + 3 * up(4 * S * T * R) + up(8 * S * (T + 1024)) + (up(2 * V * ((J + 31) // 32 * 32)) if bf16 else 0)
    for shape in ((500, 8, 50), (33, 3, 63), (33, 3, 64), (1, 1, 0), (1 << 14, 1, 1023)):
        assert k.rnnt_align_workspace_bytes(*shape) == full(*shape), shape
    for T, S, R, J, V in ((500, 8, 8, 512, 1024), (33, 3, 9, 48, 130), (1 << 18, 1, 64, 16, 2)):
        for precision in ("f32", "bf16"):
            assert k.rnnt_align_workspace_bytes(T, S, 1023, J, V, R=R, precision=precision) == band(T, S, R, J, V, precision == "bf16")
    assert full(500, 8, 50) < k.rnnt_workspace_bytes(500, 8, 50, 512, 64, want_grads=False)     # three planes and bit words against seven planes
    with pytest.raises(ValueError):
        k.rnnt_align_workspace_bytes(4, 1, 2, R=2, precision="f16")
