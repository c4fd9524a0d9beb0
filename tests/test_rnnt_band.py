"""krnnt_band_* without a GPU (include/klstm_rnnt.h, BAND-PRUNED TRAINING): the limits and argument checks, which all run before the
first HIP call, and the workspace formula of the header recomputed here."""
import ctypes

import pytest


def test_refused_shapes_and_arguments_without_a_gpu():
    import kaldi_lstm_amd as k
    lib = k.load_library()
    p = ctypes.c_void_p(256)                            # never dereferenced: refused before any pointer is followed
    big = ctypes.c_size_t(1 << 40)

    def ev(T=4, S=1, Umax=2, J=16, V=5, blank=0, R=2, enc=p, band=p, es=16, ds=16, de=p, bg=p, ws=p, nbytes=big, tot=None):
        return lib.krnnt_band_eval(enc, es, p, 16, p, p, T, S, Umax, J, V, p, p, p, blank, R, band, de, ds, p, 16, p, bg, p, tot, ws, nbytes, None)

    def fr(T=4, S=1, R=2, left=0, lens=p, band=p, frames=None):
        return lib.krnnt_band_from_frames(frames, lens, p, T, S, R, left, band, None)

    for fn, name, cases in ((ev, b"krnnt_band_eval:", [dict(S=0), dict(S=33), dict(T=0), dict(Umax=-1), dict(Umax=1024), dict(R=0), dict(R=65),
                                                      dict(T=(1 << 19) + 1, S=32, R=1), dict(T=1 << 18, R=64, S=2), dict(J=24), dict(J=1040),
                                                      dict(V=1), dict(V=4097), dict(blank=5), dict(blank=-1)]),
                            (fr, b"krnnt_band_from_frames:", [dict(S=0), dict(S=33), dict(T=0), dict(R=0), dict(R=65), dict(T=1 << 23, R=3),
                                                             dict(left=-1), dict(left=2)])):
        for kw in cases:
            assert fn(**kw) == 2 and lib.klstm_last_error().startswith(name), (name, kw)        # KLSTM_ERR_SHAPE
    for kw in (dict(enc=None), dict(band=None), dict(ws=None), dict(es=15), dict(ds=15), dict(de=None), dict(bg=None), dict(enc=ctypes.c_void_p(258)),
               dict(band=ctypes.c_void_p(258)), dict(tot=ctypes.c_void_p(260)), dict(ws=ctypes.c_void_p(264)),
               dict(nbytes=ctypes.c_size_t(lib.krnnt_band_workspace_bytes(4, 1, 2, 2, 16, 5) - 1))):
        assert ev(**kw) == 1 and lib.klstm_last_error().startswith(b"krnnt_band_eval:"), kw     # KLSTM_ERR_ARG
    for kw in (dict(lens=None), dict(band=None), dict(frames=ctypes.c_void_p(258))):
        assert fr(**kw) == 1 and lib.klstm_last_error().startswith(b"krnnt_band_from_frames:"), kw
    assert lib.krnnt_band_workspace_bytes(1 << 20, 1, 1023, 16, 512, 64) > 0                      # 2^20 frames of 1024 positions: krnnt_eval refuses
    assert lib.krnnt_workspace_bytes(1 << 20, 1, 1023, 512, 64) == 0
    assert lib.krnnt_band_forward_workspace_bytes(4, 1, 65) == 0 and lib.klstm_last_error().startswith(b"krnnt_band_forward_workspace_bytes:")
    with pytest.raises(k.KlstmError) as ei:
        k.rnnt_band_workspace_bytes(4, 1, 2, 2, 24, 5, want_grads=False)                         # J is checked without gradients too
    assert ei.value.status == 2


def test_workspace_is_the_documented_formula():
    import kaldi_lstm_amd as k
    up = lambda v: (v + 255) // 256 * 256

    def formula(T, S, Umax, R, J, V):
        N, tb, splits = S * T * R, (T + 15) // 16, k.rnnt_grad_splits(J, V)
        nodes = up(16 * S) + up(8 * S) + up(16 * S * (T + 1024)) + 7 * up(4 * N)
        partials = up(4 * S * ((Umax + 1) + tb * R) * J) + up(4 * splits * V * J) + up(8 * splits * V)
        return nodes, partials

    for shape in ((500, 8, 50, 8, 512, 64), (33, 3, 16, 9, 48, 130), (3000, 8, 800, 8, 512, 1024)):
        nodes, partials = formula(*shape)
        assert k.rnnt_band_workspace_bytes(*shape) == nodes + partials and k.rnnt_band_workspace_bytes(*shape, want_grads=False) == nodes
    T, S, Umax, R, J, V = 500, 8, 50, 8, 512, 64
    grow = k.rnnt_band_workspace_bytes(T, S, 2 * Umax + 1, R, J, V) - k.rnnt_band_workspace_bytes(T, S, Umax, R, J, V)
    assert grow == up(4 * S * (2 * Umax + 2 + 32 * R) * J) - up(4 * S * (Umax + 1 + 32 * R) * J)    # Umax adds (Umax+1) S J floats: no T (Umax+1) term
    assert k.rnnt_band_workspace_bytes(T, S, Umax, R, J, V) < 0.41 * k.rnnt_workspace_bytes(T, S, Umax, J, V)
