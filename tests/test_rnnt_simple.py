"""krnnt_simple_* and krnnt_band_from_occupation without a GPU (include/klstm_rnnt.h, THE SIMPLE JOINER): the limits and argument checks,
which all run before the first HIP call, and the workspace formula of the header recomputed here."""
import ctypes


def test_refused_shapes_and_arguments_without_a_gpu():
    import kaldi_lstm_amd as k
    lib = k.load_library()
    p = ctypes.c_void_p(256)                            # never dereferenced: refused before any pointer is followed
    big = ctypes.c_size_t(1 << 40)

    def ev(T=4, S=1, Umax=2, V=5, blank=0, am=p, ams=5, lens=p, dam=p, ds=5, dlm=p, occ=p, loss=p, ws=p, nbytes=big, tot=None):
        return lib.krnnt_simple_eval(am, ams, p, 5, T, S, Umax, V, lens, p, p, blank, dam, ds, dlm, 5, occ, loss, tot, ws, nbytes, None)

    def oc(T=4, S=1, Umax=2, R=2, occ=p, lens=p, band=p):
        return lib.krnnt_band_from_occupation(occ, lens, p, T, S, Umax, R, band, None)

    shapes = [dict(S=0), dict(S=33), dict(T=0), dict(Umax=-1), dict(Umax=1024), dict(T=(1 << 14) + 1, Umax=1023)]
    for fn, name, cases in ((ev, b"krnnt_simple_eval:", shapes + [dict(V=1), dict(V=4097), dict(blank=5), dict(blank=-1)]),
                            (oc, b"krnnt_band_from_occupation:", shapes + [dict(R=0), dict(R=65)])):
        for kw in cases:
            assert fn(**kw) == 2 and lib.klstm_last_error().startswith(name), (name, kw)        # KLSTM_ERR_SHAPE
    need = lib.krnnt_simple_workspace_bytes(4, 1, 2, 5)
    for kw in (dict(am=None), dict(lens=None), dict(loss=None), dict(ws=None), dict(ams=4), dict(ds=4), dict(dam=None), dict(dlm=None),
               dict(am=ctypes.c_void_p(258)), dict(occ=ctypes.c_void_p(258)), dict(tot=ctypes.c_void_p(260)), dict(ws=ctypes.c_void_p(264)),
               dict(nbytes=ctypes.c_size_t(need - 1))):
        assert ev(**kw) == 1 and lib.klstm_last_error().startswith(b"krnnt_simple_eval:"), kw   # KLSTM_ERR_ARG
    for kw in (dict(occ=None), dict(lens=None), dict(band=None), dict(occ=ctypes.c_void_p(258))):
        assert oc(**kw) == 1 and lib.klstm_last_error().startswith(b"krnnt_band_from_occupation:"), kw
    assert lib.krnnt_simple_workspace_bytes(4, 1, 2, 4097) == 0 and lib.klstm_last_error().startswith(b"krnnt_simple_workspace_bytes:")


def test_workspace_is_the_documented_formula_and_has_no_node_times_class_term():
    import kaldi_lstm_amd as k
    up = lambda v: (v + 255) // 256 * 256

    def formula(T, S, Umax, V):
        N, Vp, U1 = S * T * (Umax + 1), (V + 31) // 32 * 32, Umax + 1
        return (up(16 * S) + up(8 * S) + up(16 * S * (T + U1)) + 7 * up(4 * N) + up(4 * S * T * Vp) + up(4 * S * U1 * Vp) + up(4 * S * T)
                + up(4 * S * U1))

    for shape in ((500, 8, 50, 1024), (33, 3, 63, 130), (1, 1, 0, 2)):
        assert k.rnnt_simple_workspace_bytes(*shape) == formula(*shape), shape
    T, S, Umax, V = 1 << 14, 1, 1023, 4096                                     # 2^24 nodes of 4096 classes: an N V array would be 256 GiB
    got = k.rnnt_simple_workspace_bytes(T, S, Umax, V)
    assert 0 < got == formula(T, S, Umax, V) < (4 * T * (Umax + 1) * V) // 256
