"""RNN-transducer training (full lattice and band-pruned), greedy decoding and beam search on torch CUDA tensors: the krnnt_* entries of include/klstm_rnnt.h (which defines every
quantity; the torch yardsticks: tests/rnnt_ref.py, tests/rnnt_band_ref.py, tests/rnnt_greedy_ref.py, tests/rnnt_beam_ref.py).  Plumbing only, no arithmetic: the label lists become the CSR arrays of the
C-ABI through ctc.py's helpers, the workspace is cached per shape; without the library or a GPU the calls raise."""
import ctypes

from .binding import _chk, _sp, load_library
from .ctc import _check_totals, _packed, _ptr, _workspace, _workspace_bytes


def rnnt_workspace_bytes(T, S, Umax, J, V, want_grads=True):
    """bytes of workspace krnnt_eval needs; without gradients the reduction partials are left out (J and V do not matter then)"""
    if not want_grads:
        rnnt_workspace_bytes(T, S, Umax, J, V)           # the limits on J and V still hold
        return _workspace_bytes("krnnt_forward_workspace_bytes", T, S, Umax)
    return _workspace_bytes("krnnt_workspace_bytes", T, S, Umax, J, V)


def rnnt_grad_splits(J, V):
    return int(load_library().krnnt_grad_splits(int(J), int(V)))


def _rows(t, cols=None):
    import torch
    assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and (cols is None or t.shape[1] == cols)
    return t


def rnnt_eval(enc, pred, W, b, lens, labels, blank=0, want_grads=True, totals=None, stream=None, out=None):
    """enc [T*S, J] (row t*S + s), pred [(Umax+1)*S, J] (row u*S + s): float32 CUDA, any row stride; W [V, J], b [V] contiguous; lens:
    S lengths (a sequence or an int32 CUDA tensor); labels: a list of S label sequences, or what pack_labels() returned.  Returns a
    dict: loss [S] float32 (0 for an idle or rejected stream) and, with want_grads, d_enc, d_pred (like enc, pred), W_grad, b_grad.
    out: a dict of preallocated d_enc / d_pred / W_grad / b_grad to write into (rows of rejected streams are left as they are).
    totals: a float64[5] CUDA tensor that loss sum, frames, labels, streams done and streams rejected are added to.  Nothing
    synchronises."""
    import torch
    lib, dev = load_library(), enc.device
    _rows(enc)
    J = enc.shape[1]
    _rows(pred, J)
    assert W.is_cuda and W.dtype == torch.float32 and W.dim() == 2 and W.is_contiguous() and W.shape[1] == J
    V = W.shape[0]
    assert b.is_cuda and b.dtype == torch.float32 and b.is_contiguous() and b.numel() == V
    if isinstance(lens, torch.Tensor) and lens.is_cuda:
        assert lens.dtype == torch.int32 and lens.is_contiguous()
        lens_dev = lens
    else:
        lens_dev = torch.tensor([int(v) for v in lens], dtype=torch.int32, device=dev)
    S = lens_dev.numel()
    assert S > 0 and enc.shape[0] % S == 0 and pred.shape[0] % S == 0, "rows must be T * len(lens) and (Umax + 1) * len(lens)"
    T, Umax = enc.shape[0] // S, pred.shape[0] // S - 1
    lab_dev, off_dev, _ = _packed(labels, S, dev)
    _check_totals(totals, 5)
    nbytes = rnnt_workspace_bytes(T, S, Umax, J, V, want_grads)
    ws = _workspace("rnnt", (T, S, Umax, J, V, bool(want_grads)), nbytes, dev)
    res = {"loss": torch.empty(S, device=dev)}
    g = [None] * 4
    if want_grads:
        out = out or {}
        g = [out.get("d_enc"), out.get("d_pred"), out.get("W_grad"), out.get("b_grad")]
        g = [t if t is not None else torch.empty(shape, device=dev)
             for t, shape in zip(g, [(T * S, J), ((Umax + 1) * S, J), (V, J), (V,)])]
        _rows(g[0], J), _rows(g[1], J)
        assert g[0].shape[0] == T * S and g[1].shape[0] == (Umax + 1) * S and g[2].is_contiguous() and g[2].shape == (V, J) and g[3].numel() == V
        res.update(d_enc=g[0], d_pred=g[1], W_grad=g[2], b_grad=g[3])
    _chk(lib.krnnt_eval(enc.data_ptr(), enc.stride(0), pred.data_ptr(), pred.stride(0), W.data_ptr(), b.data_ptr(), T, S, Umax, J, V,
                        lens_dev.data_ptr(), lab_dev.data_ptr(), off_dev.data_ptr(), int(blank), _ptr(g[0]), g[0].stride(0) if want_grads else 0,
                        _ptr(g[1]), g[1].stride(0) if want_grads else 0, _ptr(g[2]), _ptr(g[3]), res["loss"].data_ptr(), _ptr(totals),
                        ws.data_ptr(), ctypes.c_size_t(nbytes), _sp(stream)))
    return res


def _band_precision(precision):
    if precision not in ("f32", "bf16"):
        raise ValueError("precision %r: the band-pruned joint runs in 'f32' or 'bf16'" % (precision,))
    return precision == "bf16"


def rnnt_band_workspace_bytes(T, S, Umax, R, J, V, want_grads=True, precision="f32"):
    """bytes of workspace krnnt_band_eval needs (include/klstm_rnnt.h gives the formula: no term in T (Umax+1)); without gradients
    Umax, J and V do not enter it.  precision "bf16": what krnnt_band_eval_bf16 needs (the bf16 copies of W on top)"""
    if _band_precision(precision):
        return _workspace_bytes("krnnt_band_bf16_workspace_bytes", T, S, Umax, R, J, V, bool(want_grads))
    full = _workspace_bytes("krnnt_band_workspace_bytes", T, S, Umax, R, J, V)      # the limits on Umax, J and V hold either way
    return full if want_grads else _workspace_bytes("krnnt_band_forward_workspace_bytes", T, S, R)


def _lens_dev(lens, dev):
    import torch
    if isinstance(lens, torch.Tensor) and lens.is_cuda:
        assert lens.dtype == torch.int32 and lens.is_contiguous()
        return lens
    return torch.tensor([int(v) for v in lens], dtype=torch.int32, device=dev)


def rnnt_band_from_frames(lens, labels, R, frames=None, left=None, T=None, device="cuda", stream=None):
    """band_lo [S, T] int32 for rnnt_band_eval (krnnt_band_from_frames states the rule): a valid band of width R around the alignment
    that puts label i of stream s at frame frames[s][i] (S lists like labels, or an int32 CUDA tensor packed like the labels: what
    ctc_align or the greedy decoder give), around the straight line without frames.  left: label positions kept below the
    alignment, (R-1)//2 by default.  A stream no band of width R can serve gets a row of -1 (rnnt_band_eval rejects it).
    T: the longest length by default (lens on the host)."""
    import torch
    lens_dev = _lens_dev(lens, device)
    S, dev = lens_dev.numel(), lens_dev.device
    T = max(int(v) for v in lens) if T is None else int(T)
    lab_dev, off_dev, _ = _packed(labels, S, dev)
    fr = frames
    if fr is not None and not isinstance(fr, torch.Tensor):
        assert len(fr) == S
        flat = [int(f) for row in fr for f in row]      # no label at all: nothing to pack, and the straight line is the same band
        fr = torch.tensor(flat, dtype=torch.int32, device=dev) if flat else None
    if fr is not None:
        assert fr.is_cuda and fr.dtype == torch.int32 and fr.is_contiguous() and fr.numel() == lab_dev.numel(), "one frame per label"
    band = torch.empty(S, max(T, 1), dtype=torch.int32, device=dev)
    _chk(load_library().krnnt_band_from_frames(_ptr(fr), lens_dev.data_ptr(), off_dev.data_ptr(), T, S, int(R),
                                               (int(R) - 1) // 2 if left is None else int(left), band.data_ptr(), _sp(stream)))
    return band


def rnnt_band_eval(enc, pred, W, b, lens, labels, band_lo, R, blank=0, want_grads=True, totals=None, stream=None, out=None, precision="f32"):
    """rnnt_eval inside a band: band_lo [S, T] int32 CUDA (rnnt_band_from_frames, or any valid band: klstm_rnnt.h) and its width R.
    Arguments and the returned dict are those of rnnt_eval; a stream whose band is not valid is rejected like one with a bad label.
    precision "bf16": the three joint products on the bf16 matrix instruction (krnnt_band_eval_bf16; klstm_rnnt.h, THE BF16 JOINT)."""
    import torch
    bf16 = _band_precision(precision)
    lib, dev = load_library(), enc.device
    _rows(enc)
    J = enc.shape[1]
    _rows(pred, J)
    assert W.is_cuda and W.dtype == torch.float32 and W.dim() == 2 and W.is_contiguous() and W.shape[1] == J
    V = W.shape[0]
    assert b.is_cuda and b.dtype == torch.float32 and b.is_contiguous() and b.numel() == V
    lens_dev = _lens_dev(lens, dev)
    S = lens_dev.numel()
    assert S > 0 and enc.shape[0] % S == 0 and pred.shape[0] % S == 0, "rows must be T * len(lens) and (Umax + 1) * len(lens)"
    T, Umax, R = enc.shape[0] // S, pred.shape[0] // S - 1, int(R)
    assert band_lo.is_cuda and band_lo.dtype == torch.int32 and band_lo.is_contiguous() and tuple(band_lo.shape) == (S, T)
    lab_dev, off_dev, _ = _packed(labels, S, dev)
    _check_totals(totals, 5)
    nbytes = rnnt_band_workspace_bytes(T, S, Umax, R, J, V, want_grads, precision)
    ws = _workspace("rnnt_band", (T, S, Umax, R, J, V, bool(want_grads), precision), nbytes, dev)
    res = {"loss": torch.empty(S, device=dev)}
    g = [None] * 4
    if want_grads:
        out = out or {}
        g = [out.get("d_enc"), out.get("d_pred"), out.get("W_grad"), out.get("b_grad")]
        g = [t if t is not None else torch.empty(shape, device=dev)
             for t, shape in zip(g, [(T * S, J), ((Umax + 1) * S, J), (V, J), (V,)])]
        _rows(g[0], J), _rows(g[1], J)
        assert g[0].shape[0] == T * S and g[1].shape[0] == (Umax + 1) * S and g[2].is_contiguous() and g[2].shape == (V, J) and g[3].numel() == V
        res.update(d_enc=g[0], d_pred=g[1], W_grad=g[2], b_grad=g[3])
    entry = lib.krnnt_band_eval_bf16 if bf16 else lib.krnnt_band_eval
    _chk(entry(enc.data_ptr(), enc.stride(0), pred.data_ptr(), pred.stride(0), W.data_ptr(), b.data_ptr(), T, S, Umax, J, V,
               lens_dev.data_ptr(), lab_dev.data_ptr(), off_dev.data_ptr(), int(blank), R, band_lo.data_ptr(), _ptr(g[0]),
               g[0].stride(0) if want_grads else 0, _ptr(g[1]), g[1].stride(0) if want_grads else 0, _ptr(g[2]), _ptr(g[3]),
               res["loss"].data_ptr(), _ptr(totals), ws.data_ptr(), ctypes.c_size_t(nbytes), _sp(stream)))
    return res


def rnnt_align_workspace_bytes(T, S, Umax, J=16, V=2, R=None, precision="f32"):
    """bytes of workspace krnnt_align needs (R None: the full lattice; J and V do not enter it) or krnnt_band_align (width R; J and V
    enter with precision "bf16" only); include/klstm_rnnt.h, FORCED ALIGNMENT, gives both formulas"""
    if R is None:
        return _workspace_bytes("krnnt_align_workspace_bytes", T, S, Umax)
    return _workspace_bytes("krnnt_band_align_workspace_bytes", T, S, R, J, V, _band_precision(precision))


def rnnt_align(enc, pred, W, b, lens, labels, blank=0, band_lo=None, R=None, precision="f32", want_logp=False, stream=None):
    """The best alignment of the labels (klstm_rnnt.h, FORCED ALIGNMENT): enc, pred, W, b, lens, labels as in rnnt_eval.  band_lo None:
    the full lattice (krnnt_align); band_lo [S, T] int32 CUDA with its width R: inside that band (krnnt_band_align), precision "bf16":
    with the bf16 joint's log-probabilities.  Returns a dict: frames, int32 CUDA, one frame per label packed like the labels (what
    rnnt_band_from_frames takes as frames=); score [S] float32, the log-probability of the best path (0: idle or rejected); logp,
    the label steps' log-probabilities packed like frames (None without want_logp).  The entries of a rejected stream stay as
    allocated (zeros).  Nothing synchronises."""
    import torch
    bf16 = _band_precision(precision)
    if band_lo is None and bf16:
        raise ValueError("precision 'bf16': only the band-pruned joint has a bf16 variant; give band_lo and R")
    lib, dev = load_library(), enc.device
    _rows(enc)
    J = enc.shape[1]
    _rows(pred, J)
    assert W.is_cuda and W.dtype == torch.float32 and W.dim() == 2 and W.is_contiguous() and W.shape[1] == J
    V = W.shape[0]
    assert b.is_cuda and b.dtype == torch.float32 and b.is_contiguous() and b.numel() == V
    lens_dev = _lens_dev(lens, dev)
    S = lens_dev.numel()
    assert S > 0 and enc.shape[0] % S == 0 and pred.shape[0] % S == 0, "rows must be T * len(lens) and (Umax + 1) * len(lens)"
    T, Umax = enc.shape[0] // S, pred.shape[0] // S - 1
    lab_dev, off_dev, _ = _packed(labels, S, dev)
    frames = torch.zeros(lab_dev.numel(), dtype=torch.int32, device=dev)
    logp = torch.zeros(lab_dev.numel(), device=dev) if want_logp else None
    score = torch.empty(S, device=dev)
    head = (enc.data_ptr(), enc.stride(0), pred.data_ptr(), pred.stride(0), W.data_ptr(), b.data_ptr(), T, S, Umax, J, V, lens_dev.data_ptr(),
            lab_dev.data_ptr(), off_dev.data_ptr(), int(blank))
    if band_lo is None:
        nbytes = rnnt_align_workspace_bytes(T, S, Umax)
        ws = _workspace("rnnt_align", (T, S, Umax), nbytes, dev)
        _chk(lib.krnnt_align(*head, frames.data_ptr(), _ptr(logp), score.data_ptr(), ws.data_ptr(), ctypes.c_size_t(nbytes), _sp(stream)))
    else:
        R = int(R)
        assert band_lo.is_cuda and band_lo.dtype == torch.int32 and band_lo.is_contiguous() and tuple(band_lo.shape) == (S, T)
        nbytes = rnnt_align_workspace_bytes(T, S, Umax, J, V, R, precision)
        ws = _workspace("rnnt_band_align", (T, S, R, J, V, precision), nbytes, dev)
        _chk(lib.krnnt_band_align(*head, R, band_lo.data_ptr(), int(bf16), frames.data_ptr(), _ptr(logp), score.data_ptr(), ws.data_ptr(),
                                  ctypes.c_size_t(nbytes), _sp(stream)))
    return dict(frames=frames, score=score, logp=logp)


def rnnt_simple_workspace_bytes(T, S, Umax, V):
    """bytes of workspace krnnt_simple_eval needs (include/klstm_rnnt.h gives the formula: no term in T (Umax+1) V)"""
    return _workspace_bytes("krnnt_simple_workspace_bytes", T, S, Umax, V)


def rnnt_simple_eval(am, lm, lens, labels, blank=0, want_grads=True, want_occ=False, totals=None, stream=None, out=None):
    """The additive simple-joiner loss (klstm_rnnt.h, THE SIMPLE JOINER): am [T*S, V] (row t*S + s), lm [(Umax+1)*S, V] (row u*S + s),
    float32 CUDA, any row stride; lens, labels, totals as in rnnt_eval.  Returns a dict: loss [S] and, with want_grads, d_am, d_lm
    (like am, lm); with want_occ, occ [S, T, Umax+1], the node posteriors that rnnt_band_from_occupation turns into a band.
    out: a dict of preallocated d_am / d_lm / occ (the parts of rejected streams are left as they are).  Nothing synchronises."""
    import torch
    lib, dev = load_library(), am.device
    _rows(am)
    V = am.shape[1]
    _rows(lm, V)
    lens_dev = _lens_dev(lens, dev)
    S = lens_dev.numel()
    assert S > 0 and am.shape[0] % S == 0 and lm.shape[0] % S == 0, "rows must be T * len(lens) and (Umax + 1) * len(lens)"
    T, Umax = am.shape[0] // S, lm.shape[0] // S - 1
    lab_dev, off_dev, _ = _packed(labels, S, dev)
    _check_totals(totals, 5)
    nbytes = rnnt_simple_workspace_bytes(T, S, Umax, V)
    ws = _workspace("rnnt_simple", (T, S, Umax, V), nbytes, dev)
    res, out = {"loss": torch.empty(S, device=dev)}, out or {}
    g, occ = [None, None], None
    if want_grads:
        g = [out.get("d_am"), out.get("d_lm")]
        g = [t if t is not None else torch.empty(shape, device=dev) for t, shape in zip(g, [(T * S, V), ((Umax + 1) * S, V)])]
        _rows(g[0], V), _rows(g[1], V)
        assert g[0].shape[0] == T * S and g[1].shape[0] == (Umax + 1) * S
        res.update(d_am=g[0], d_lm=g[1])
    if want_occ:
        occ = out.get("occ")
        occ = occ if occ is not None else torch.empty(S, T, Umax + 1, device=dev)
        assert occ.is_cuda and occ.dtype == torch.float32 and occ.is_contiguous() and tuple(occ.shape) == (S, T, Umax + 1)
        res["occ"] = occ
    _chk(lib.krnnt_simple_eval(am.data_ptr(), am.stride(0), lm.data_ptr(), lm.stride(0), T, S, Umax, V, lens_dev.data_ptr(), lab_dev.data_ptr(),
                               off_dev.data_ptr(), int(blank), _ptr(g[0]), g[0].stride(0) if want_grads else 0, _ptr(g[1]),
                               g[1].stride(0) if want_grads else 0, _ptr(occ), res["loss"].data_ptr(), _ptr(totals), ws.data_ptr(),
                               ctypes.c_size_t(nbytes), _sp(stream)))
    return res


def rnnt_band_from_occupation(occ, lens, labels, R, stream=None):
    """band_lo [S, T] int32 for rnnt_band_eval from node occupations occ [S, T, Umax+1] float32 CUDA (rnnt_simple_eval's): per frame the
    R label positions that hold the most mass, made monotone and connected (krnnt_band_from_occupation states the rule).  A stream no
    band of width R can serve gets a row of -1."""
    import torch
    assert occ.is_cuda and occ.dtype == torch.float32 and occ.dim() == 3 and occ.is_contiguous()
    S, T, U1 = occ.shape
    lens_dev = _lens_dev(lens, occ.device)
    assert lens_dev.numel() == S
    _, off_dev, _ = _packed(labels, S, occ.device)
    band = torch.empty(S, T, dtype=torch.int32, device=occ.device)
    _chk(load_library().krnnt_band_from_occupation(occ.data_ptr(), lens_dev.data_ptr(), off_dev.data_ptr(), T, S, U1 - 1, int(R),
                                                   band.data_ptr(), _sp(stream)))
    return band


def rnnt_pack(labels, S, V, bos, embed=None, bias=None, Umax=None, device="cuda", stream=None):
    """The prediction network's input [(Umax+1)*S, width], row u*S + s from x_u (x_0 = bos, x_u = y_u): the one-hot over V columns, or
    with embed [D, V] (and bias [D]) the gathered column plus bias; rows without an input are zeros.  labels: S label sequences or
    what pack_labels() returned; Umax: the longest by default."""
    import torch
    lab_dev, off_dev, longest = _packed(labels, S, device)
    Umax = longest if Umax is None else int(Umax)
    D = 0
    if embed is not None:
        assert embed.is_cuda and embed.dtype == torch.float32 and embed.is_contiguous() and embed.dim() == 2 and embed.shape[1] == V
        D = embed.shape[0]
        assert bias is None or (bias.is_cuda and bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == D)
    out = torch.empty((Umax + 1) * S, D if embed is not None else V, device=lab_dev.device)
    _chk(load_library().krnnt_pack(lab_dev.data_ptr(), off_dev.data_ptr(), int(S), Umax, int(V), int(bos), _ptr(embed), _ptr(bias), D,
                                   out.data_ptr(), out.stride(0), _sp(stream)))
    return out


def rnnt_greedy_state_bytes(T, S, J):
    """bytes of state krnnt_greedy_begin / krnnt_greedy_step need (include/klstm_rnnt.h: per stream and per chunk of frames)"""
    return _workspace_bytes("krnnt_greedy_state_bytes", T, S, J)


def _embedding(embed, bias, V):
    import torch
    if embed is None:
        return 0
    assert embed.is_cuda and embed.dtype == torch.float32 and embed.is_contiguous() and embed.dim() == 2 and embed.shape[1] == V
    assert bias is None or (bias.is_cuda and bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == embed.shape[0])
    return embed.shape[0]


def rnnt_greedy_begin(T, S, J, V, bos, lens_dev, next_in, state, embed=None, bias=None, stream=None):
    """Start a greedy decode of S streams (lens_dev: int32 CUDA lengths): the state is reset and next_in [S, V or D] gets the rows of bos."""
    D = _embedding(embed, bias, V)
    _chk(load_library().krnnt_greedy_begin(int(T), int(S), int(J), int(V), int(bos), lens_dev.data_ptr(), _ptr(embed), _ptr(bias), D,
                                           _rows(next_in).data_ptr(), next_in.stride(0), state.data_ptr(), ctypes.c_size_t(state.numel()), _sp(stream)))


def rnnt_greedy_step(enc, pred_rows, W, b, T, S, blank, max_symbols, next_in, hyp, hyp_len, frames, score, flags, live, state,
                     embed=None, bias=None, stream=None):
    """Step u of all streams: pred_rows [S, J] are the predictor's outputs for next_in; one more label (hyp / frames [S, max_len] int32,
    hyp_len [S]) per live stream, score [S] float32, flags [S] and live [1] int32 updated, next_in rewritten.  Nothing synchronises."""
    J, V = _rows(enc).shape[1], W.shape[0]
    _rows(pred_rows, J)
    D = _embedding(embed, bias, V)
    _chk(load_library().krnnt_greedy_step(enc.data_ptr(), enc.stride(0), pred_rows.data_ptr(), pred_rows.stride(0), W.data_ptr(), b.data_ptr(),
                                          int(T), int(S), J, V, int(blank), int(max_symbols), hyp.shape[1], _ptr(embed), _ptr(bias), D,
                                          _rows(next_in).data_ptr(), next_in.stride(0), hyp.data_ptr(), hyp_len.data_ptr(), _ptr(frames),
                                          score.data_ptr(), flags.data_ptr(), live.data_ptr(), state.data_ptr(), ctypes.c_size_t(state.numel()),
                                          _sp(stream)))


def rnnt_greedy_decode(enc, lens, W, b, predictor, bos, blank=0, max_symbols=10, max_len=255, embed=None, bias=None, poll_every=8,
                       stream=None):
    """Greedy transducer decoding of enc [T*S, J] (row t*S + s; lens: S lengths).  predictor: a callable from the next-input rows
    [S, V] (one-hot; [S, D] with embed [D, V]) to [S, J] float32 CUDA rows that carries its own state from call to call and starts
    from reset state.  At most max_len + 1 steps; the number of live streams is read back every poll_every steps (0: never).
    Returns a dict: tokens, frames (S lists), score [S] float32, flags [S] int32 (klstm_rnnt.h), steps."""
    import torch
    dev = enc.device
    assert W.is_cuda and W.dtype == torch.float32 and W.is_contiguous() and b.is_cuda and b.dtype == torch.float32 and b.is_contiguous()
    lens_dev = lens if isinstance(lens, torch.Tensor) and lens.is_cuda else torch.tensor([int(v) for v in lens], dtype=torch.int32, device=dev)
    assert lens_dev.dtype == torch.int32 and lens_dev.is_contiguous()
    S, (V, J) = lens_dev.numel(), W.shape
    assert S > 0 and enc.shape[0] % S == 0 and enc.shape[1] == J and b.numel() == V
    T = enc.shape[0] // S
    nbytes = rnnt_greedy_state_bytes(T, S, J)
    state = _workspace("rnnt_greedy", (T, S, J), nbytes, dev)[:nbytes]
    ints = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
    next_in = torch.empty(S, embed.shape[0] if embed is not None else V, device=dev)
    hyp, frames, hyp_len, flags, live, score = ints(S, max_len), ints(S, max_len), ints(S), ints(S), ints(1), torch.zeros(S, device=dev)
    rnnt_greedy_begin(T, S, J, V, bos, lens_dev, next_in, state, embed, bias, stream)
    steps = 0
    while steps < max_len + 1:
        rnnt_greedy_step(enc, predictor(next_in), W, b, T, S, blank, max_symbols, next_in, hyp, hyp_len, frames, score, flags, live, state,
                         embed, bias, stream)
        steps += 1
        if poll_every and steps % poll_every == 0 and int(live) == 0:
            break
    n, h, f = hyp_len.tolist(), hyp.tolist(), frames.tolist()
    return dict(tokens=[h[s][:n[s]] for s in range(S)], frames=[f[s][:n[s]] for s in range(S)], score=score, flags=flags, steps=steps)


def rnnt_beam_state_bytes(T, S, B, J, V):
    """bytes of state krnnt_beam_begin / krnnt_beam_step need (include/klstm_rnnt.h gives the formula)"""
    return _workspace_bytes("krnnt_beam_state_bytes", T, S, B, J, V)


def rnnt_beam_begin(T, S, B, J, V, bos, lens_dev, next_in, parents, state, embed=None, bias=None, stream=None):
    """Start a beam search of S streams with B slots each: the state is reset, next_in [S*B, V or D] gets the bos row in slot 0 of every
    live stream and parents [S*B] int32 gets -1."""
    D = _embedding(embed, bias, V)
    _chk(load_library().krnnt_beam_begin(int(T), int(S), int(B), int(J), int(V), int(bos), lens_dev.data_ptr(), _ptr(embed), _ptr(bias), D,
                                         _rows(next_in).data_ptr(), next_in.stride(0), parents.data_ptr(), state.data_ptr(),
                                         ctypes.c_size_t(state.numel()), _sp(stream)))


def rnnt_beam_step(enc, pred_rows, W, b, T, S, B, blank, next_in, parents, hyp, hyp_len, score, count, flags, live, state, embed=None,
                   bias=None, stream=None):
    """Step u of all streams: pred_rows [S*B, J] are the predictor's outputs for next_in (row s*B + b: slot b of stream s).  The lists
    (hyp [S, N, max_len], hyp_len / score [S, N], count [S]), flags [S] and live [1] are updated; next_in and parents (the row of
    pred_rows each new slot continues, -1: empty) are rewritten.  Nothing synchronises."""
    J, V = _rows(enc).shape[1], W.shape[0]
    _rows(pred_rows, J)
    D = _embedding(embed, bias, V)
    _chk(load_library().krnnt_beam_step(enc.data_ptr(), enc.stride(0), pred_rows.data_ptr(), pred_rows.stride(0), W.data_ptr(), b.data_ptr(),
                                        int(T), int(S), int(B), hyp.shape[1], J, V, int(blank), hyp.shape[2], _ptr(embed), _ptr(bias), D,
                                        _rows(next_in).data_ptr(), next_in.stride(0), parents.data_ptr(), hyp.data_ptr(), hyp_len.data_ptr(),
                                        score.data_ptr(), count.data_ptr(), flags.data_ptr(), live.data_ptr(), state.data_ptr(),
                                        ctypes.c_size_t(state.numel()), _sp(stream)))


def rnnt_beam_decode(enc, lens, pred_fn, W, b, bos, blank=0, beam=4, nbest=None, max_len=255, embed=None, bias=None, poll_every=8,
                     stream=None, on_step=None):
    """Transducer beam search of enc [T*S, J] (row t*S + s; lens: S lengths) with n-best lists scored by the full-sum probability.
    pred_fn(next_in, parents): from the next-input rows [S*beam, V] (one-hot; [S*beam, D] with embed [D, V]) and the int32 rows
    [S*beam] each one continues (-1: from reset state) to [S*beam, J] float32 CUDA rows; an LSTM predictor calls
    Engine.gather_state(parents) and propagates.  At most max_len + 1 steps; the number of live slots is read back every poll_every
    steps (0: never).  on_step(parents, flags, count), if given, sees the device arrays after every step.
    Returns a dict: nbest (per stream a list of (tokens, score)), score [S, N] float32, count [S], flags [S] int32, steps."""
    import torch
    dev = enc.device
    assert W.is_cuda and W.dtype == torch.float32 and W.is_contiguous() and b.is_cuda and b.dtype == torch.float32 and b.is_contiguous()
    lens_dev = lens if isinstance(lens, torch.Tensor) and lens.is_cuda else torch.tensor([int(v) for v in lens], dtype=torch.int32, device=dev)
    assert lens_dev.dtype == torch.int32 and lens_dev.is_contiguous()
    S, (V, J), B = lens_dev.numel(), W.shape, int(beam)
    N = B if nbest is None else int(nbest)
    assert S > 0 and enc.shape[0] % S == 0 and enc.shape[1] == J and b.numel() == V
    T = enc.shape[0] // S
    nbytes = rnnt_beam_state_bytes(T, S, B, J, V)
    state = _workspace("rnnt_beam", (T, S, B, J, V), nbytes, dev)[:nbytes]
    ints = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
    next_in = torch.empty(S * B, embed.shape[0] if embed is not None else V, device=dev)
    parents, hyp, hyp_len, count, flags, live = ints(S * B), ints(S, N, max_len), ints(S, N), ints(S), ints(S), ints(1)
    score = torch.zeros(S, N, device=dev)
    rnnt_beam_begin(T, S, B, J, V, bos, lens_dev, next_in, parents, state, embed, bias, stream)
    steps = 0
    while steps < max_len + 1:
        rnnt_beam_step(enc, pred_fn(next_in, parents), W, b, T, S, B, blank, next_in, parents, hyp, hyp_len, score, count, flags, live, state,
                       embed, bias, stream)
        steps += 1
        if on_step is not None:
            on_step(parents, flags, count)
        if poll_every and steps % poll_every == 0 and int(live) == 0:
            break
    n, ln, h, sc = count.tolist(), hyp_len.tolist(), hyp.tolist(), score.tolist()
    lists = [[(h[s][q][:ln[s][q]], sc[s][q]) for q in range(n[s])] for s in range(S)]
    return dict(nbest=lists, score=score, count=count, flags=flags, steps=steps)
