"""nnet1's convolutional and max-pooling components and the activations between them, over the kcnn_* entries of include/klstm_cnn.h
(which defines every quantity; the numpy yardsticks: tests/cnn_ref.py).  Plumbing only, no arithmetic: without the library or a GPU
the device calls raise.  Tensors are torch CUDA float32 [rows, width] of any row stride (row and column windows are fine)."""
import ctypes

from .binding import _chk, _sp, load_library

SIGMOID, TANH = 0, 1


def conv_plan(in_dim, out_dim, patch_dim, patch_step, patch_stride):
    """kcnn_conv_plan: (n, P, K, F) -- spliced blocks, patches, values per patch, filters.  Host only; raises KlstmError for numbers the
    definition refuses."""
    v = [ctypes.c_int(0) for _ in range(4)]
    _chk(load_library().kcnn_conv_plan(int(in_dim), int(out_dim), int(patch_dim), int(patch_step), int(patch_stride), *[ctypes.byref(x) for x in v]))
    return tuple(x.value for x in v)


def conv_workspace_floats(rows, in_dim, out_dim, patch_dim, patch_step, patch_stride):
    return int(load_library().kcnn_conv_workspace_floats(int(rows), int(in_dim), int(out_dim), int(patch_dim), int(patch_step), int(patch_stride)))


def _mat(t, cols=None):
    import torch
    assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and (t.shape[1] == 0 or t.stride(1) == 1)
    assert cols is None or t.shape[1] == cols
    return t.data_ptr(), t.stride(0)


def _flat(t, n):
    import torch
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n
    return t.data_ptr()


def _workspace(ws, need, device):
    import torch
    if ws is None or ws.numel() < need:
        ws = torch.empty(max(need, 1), dtype=torch.float32, device=device)
    assert ws.is_cuda and ws.dtype == torch.float32 and ws.is_contiguous()
    return ws


def conv_propagate(x, filters, bias, out, geometry, stream=None):
    """out[r, p F + f] = bias[f] + sum_k patch(r,p)[k] filters[f,k].  geometry = (patch_dim, patch_step, patch_stride)."""
    pd, ps, st = geometry
    n, P, K, F = conv_plan(x.shape[1], out.shape[1], pd, ps, st)
    (xp, xs), (op, os_) = _mat(x), _mat(out)
    assert x.shape[0] == out.shape[0]
    _chk(load_library().kcnn_conv_propagate(xp, xs, x.shape[0], x.shape[1], out.shape[1], pd, ps, st, _flat(filters, F * K), _flat(bias, F), op, os_, _sp(stream)))
    return out


def conv_backpropagate(out_diff, filters, in_diff, geometry, stream=None):
    """in_diff = the overlap-add over the patches of out_diff filters; in_diff None: not wanted (nothing runs)."""
    if in_diff is None:
        return None
    pd, ps, st = geometry
    n, P, K, F = conv_plan(in_diff.shape[1], out_diff.shape[1], pd, ps, st)
    (dp, ds), (ip, is_) = _mat(out_diff), _mat(in_diff)
    assert out_diff.shape[0] == in_diff.shape[0]
    _chk(load_library().kcnn_conv_backpropagate(dp, ds, out_diff.shape[0], in_diff.shape[1], out_diff.shape[1], pd, ps, st, _flat(filters, F * K), ip, is_, _sp(stream)))
    return in_diff


def conv_gradient(x, out_diff, filters_grad, bias_grad, geometry, ws=None, stream=None):
    """The pure gradient into filters_grad [F, K] and bias_grad [F] (overwritten); bit-identical from run to run, whatever the strides.
    ws: a float32 CUDA tensor of at least conv_workspace_floats(...) elements, or None: one is allocated for the call."""
    pd, ps, st = geometry
    n, P, K, F = conv_plan(x.shape[1], out_diff.shape[1], pd, ps, st)
    (xp, xs), (dp, ds) = _mat(x), _mat(out_diff)
    assert x.shape[0] == out_diff.shape[0]
    ws = _workspace(ws, conv_workspace_floats(x.shape[0], x.shape[1], out_diff.shape[1], pd, ps, st), x.device)
    _chk(load_library().kcnn_conv_gradient(xp, xs, dp, ds, x.shape[0], x.shape[1], out_diff.shape[1], pd, ps, st, _flat(filters_grad, F * K),
                                           _flat(bias_grad, F), ws.data_ptr(), ws.numel(), _sp(stream)))


def conv_update(x, out_diff, filters, bias, filters_corr, bias_corr, lr, lr_bias, momentum, geometry, ws=None, stream=None):
    """corr = momentum corr + grad; filters -= lr corr; bias -= lr_bias bias_corr, in one call.  ws: as in conv_gradient."""
    pd, ps, st = geometry
    n, P, K, F = conv_plan(x.shape[1], out_diff.shape[1], pd, ps, st)
    (xp, xs), (dp, ds) = _mat(x), _mat(out_diff)
    assert x.shape[0] == out_diff.shape[0]
    ws = _workspace(ws, conv_workspace_floats(x.shape[0], x.shape[1], out_diff.shape[1], pd, ps, st), x.device)
    _chk(load_library().kcnn_conv_update(xp, xs, dp, ds, x.shape[0], x.shape[1], out_diff.shape[1], pd, ps, st, _flat(filters, F * K), _flat(bias, F),
                                         _flat(filters_corr, F * K), _flat(bias_corr, F), float(lr), float(lr_bias), float(momentum),
                                         ws.data_ptr(), ws.numel(), _sp(stream)))


def pool_propagate(x, out, geometry, stream=None):
    """geometry = (pool_size, pool_step, pool_stride)."""
    z, g, w = geometry
    (xp, xs), (op, os_) = _mat(x), _mat(out)
    assert x.shape[0] == out.shape[0]
    _chk(load_library().kcnn_pool_propagate(xp, xs, x.shape[0], x.shape[1], out.shape[1], z, g, w, op, os_, _sp(stream)))
    return out


def pool_backpropagate(x, out, out_diff, in_diff, geometry, stream=None):
    if in_diff is None:
        return None
    z, g, w = geometry
    (xp, xs), (op, os_), (dp, ds), (ip, is_) = _mat(x), _mat(out), _mat(out_diff, out.shape[1]), _mat(in_diff, x.shape[1])
    assert x.shape[0] == out.shape[0] == out_diff.shape[0] == in_diff.shape[0]
    _chk(load_library().kcnn_pool_backpropagate(xp, xs, op, os_, dp, ds, x.shape[0], x.shape[1], out.shape[1], z, g, w, ip, is_, _sp(stream)))
    return in_diff


def activation(kind, x, out, stream=None):
    (xp, xs), (op, os_) = _mat(x), _mat(out, x.shape[1])
    assert x.shape[0] == out.shape[0]
    _chk(load_library().kcnn_activation(int(kind), xp, xs, x.shape[0], x.shape[1], op, os_, _sp(stream)))
    return out


def activation_diff(kind, out, out_diff, in_diff, stream=None):
    """from the activation's OUTPUT: in_diff = out_diff y (1 - y) or out_diff (1 - y y)."""
    if in_diff is None:
        return None
    (yp, ys), (dp, ds), (ip, is_) = _mat(out), _mat(out_diff, out.shape[1]), _mat(in_diff, out.shape[1])
    assert out.shape[0] == out_diff.shape[0] == in_diff.shape[0]
    _chk(load_library().kcnn_activation_diff(int(kind), yp, ys, dp, ds, out.shape[0], out.shape[1], ip, is_, _sp(stream)))
    return in_diff


class Convolutional:
    """The <ConvolutionalComponent> of include/klstm_nnet.hpp: filters [F, K] and bias [F] on the device, momentum buffers at zero;
    forward / backward / update as Nnet::Propagate / Backpropagate drive them (update with the input and the out_diff of the step)."""

    def __init__(self, in_dim, out_dim, patch_dim, patch_step, patch_stride, filters, bias, device="cuda"):
        import torch
        self.in_dim, self.out_dim, self.geometry = int(in_dim), int(out_dim), (int(patch_dim), int(patch_step), int(patch_stride))
        self.n, self.P, self.K, self.F = conv_plan(in_dim, out_dim, patch_dim, patch_step, patch_stride)
        self.filters = torch.as_tensor(filters, dtype=torch.float32).reshape(self.F, self.K).to(device).contiguous().clone()
        self.bias = torch.as_tensor(bias, dtype=torch.float32).reshape(self.F).to(device).contiguous().clone()
        self.filters_corr, self.bias_corr = torch.zeros_like(self.filters), torch.zeros_like(self.bias)
        self._ws = None

    def forward(self, x, out=None, stream=None):
        import torch
        out = torch.empty(x.shape[0], self.out_dim, dtype=torch.float32, device=x.device) if out is None else out
        return conv_propagate(x, self.filters, self.bias, out, self.geometry, stream)

    def backward(self, out_diff, in_diff=None, want=True, stream=None):
        import torch
        if not want:
            return None
        in_diff = torch.empty(out_diff.shape[0], self.in_dim, dtype=torch.float32, device=out_diff.device) if in_diff is None else in_diff
        return conv_backpropagate(out_diff, self.filters, in_diff, self.geometry, stream)

    def gradient(self, x, out_diff, stream=None):
        import torch
        fg, bg = torch.empty_like(self.filters), torch.empty_like(self.bias)
        conv_gradient(x, out_diff, fg, bg, self.geometry, self._workspace_for(x), stream)
        return fg, bg

    def update(self, x, out_diff, lr, momentum=0.0, lr_bias=None, stream=None):
        conv_update(x, out_diff, self.filters, self.bias, self.filters_corr, self.bias_corr, lr, lr if lr_bias is None else lr_bias,
                    momentum, self.geometry, self._workspace_for(x), stream)

    def _workspace_for(self, x):
        self._ws = _workspace(self._ws, conv_workspace_floats(x.shape[0], self.in_dim, self.out_dim, *self.geometry), x.device)
        return self._ws


class MaxPooling:
    """The <MaxPoolingComponent>: backward is nnet1's rule (the equal-element mask over the pools that contain a patch, divided by
    their number) and needs the forward call's input and output."""

    def __init__(self, in_dim, out_dim, pool_size, pool_step, pool_stride):
        self.in_dim, self.out_dim, self.geometry = int(in_dim), int(out_dim), (int(pool_size), int(pool_step), int(pool_stride))

    def forward(self, x, out=None, stream=None):
        import torch
        out = torch.empty(x.shape[0], self.out_dim, dtype=torch.float32, device=x.device) if out is None else out
        return pool_propagate(x, out, self.geometry, stream)

    def backward(self, x, out, out_diff, in_diff=None, stream=None):
        import torch
        in_diff = torch.empty(x.shape[0], self.in_dim, dtype=torch.float32, device=x.device) if in_diff is None else in_diff
        return pool_backpropagate(x, out, out_diff, in_diff, self.geometry, stream)


class _Activation:
    kind = SIGMOID

    def forward(self, x, out=None, stream=None):
        import torch
        return activation(self.kind, x, torch.empty_like(x) if out is None else out, stream)

    def backward(self, out, out_diff, in_diff=None, stream=None):
        import torch
        return activation_diff(self.kind, out, out_diff, torch.empty_like(out_diff) if in_diff is None else in_diff, stream)


class Sigmoid(_Activation):
    kind = SIGMOID


class Tanh(_Activation):
    kind = TANH
