"""RNN-transducer training on torch CUDA tensors: the krnnt_* entries of include/klstm_rnnt.h (which defines every quantity;
INTEGRATION.md 3r; the torch yardstick: tests/rnnt_ref.py).  Plumbing only, no arithmetic: the label lists become the CSR arrays of the
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
