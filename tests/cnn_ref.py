"""The numpy yardsticks of include/klstm_cnn.h (which states the definitions), both from one recipe run in two precisions:
  truth64  dtype = np.float64: the definitions in float64 from float32 inputs
  twin32   dtype = np.float32: the plain float32 recipe -- patches gathered, np.matmul in float32
The pooling rules compare and select; they are exact in both, and the float32 run is the bit-for-bit twin of the kernels."""
import numpy as np

SIGMOID, TANH = 0, 1


def conv_numbers(in_dim, out_dim, pd, ps, st):
    """(n, P, K, F), or None for numbers the definition refuses"""
    if min(in_dim, out_dim, pd, ps, st) < 1 or in_dim % st or pd > st or (st - pd) % ps:
        return None
    P = 1 + (st - pd) // ps
    if out_dim % P:
        return None
    return in_dim // st, P, (in_dim // st) * pd, out_dim // P


def patches(x, pd, ps, st):
    """[rows, D_in] -> [rows, P, K]: patch(r,p)[s pd + d] = x[r, s st + p ps + d]"""
    rows, in_dim = x.shape
    n, P = in_dim // st, 1 + (st - pd) // ps
    idx = np.arange(P)[:, None] * ps + np.arange(pd)[None, :]                 # [P, pd]
    g = x.reshape(rows, n, st)[:, :, idx]                                     # [rows, n, P, pd]
    return np.ascontiguousarray(g.transpose(0, 2, 1, 3)).reshape(rows, P, n * pd)


def conv_forward(x, filters, bias, geom, dtype):
    pd, ps, st = geom
    pt = patches(x.astype(dtype), pd, ps, st)
    rows, P, K = pt.shape
    out = np.matmul(pt.reshape(rows * P, K), np.ascontiguousarray(filters.astype(dtype).T)) + bias.astype(dtype)
    return out.reshape(rows, P * filters.shape[0])


def conv_backward(out_diff, filters, geom, in_dim, dtype):
    pd, ps, st = geom
    F, K = filters.shape
    rows, n, P = out_diff.shape[0], in_dim // st, out_diff.shape[1] // F
    G = np.matmul(out_diff.astype(dtype).reshape(rows * P, F), filters.astype(dtype)).reshape(rows, P, n, pd)
    ind = np.zeros((rows, n, st), dtype)
    for p in range(P):
        ind[:, :, p * ps:p * ps + pd] += G[:, p]
    return ind.reshape(rows, in_dim)


def conv_gradient(x, out_diff, geom, F, dtype):
    pd, ps, st = geom
    pt = patches(x.astype(dtype), pd, ps, st)
    rows, P, K = pt.shape
    od = out_diff.astype(dtype).reshape(rows * P, F)
    return np.matmul(np.ascontiguousarray(od.T), pt.reshape(rows * P, K)), od.sum(axis=0, dtype=dtype)


def sgd_step(param, corr, grad, lr, momentum, dtype):
    """the affine rule: corr = momentum corr + grad; param -= lr corr, with lr and momentum the floats the entries take.  Returns
    (param, corr)."""
    corr = dtype(np.float32(momentum)) * corr.astype(dtype) + grad.astype(dtype)
    return param.astype(dtype) - dtype(np.float32(lr)) * corr, corr


def pool_numbers(in_dim, out_dim, z, g, w):
    """(Pin, Q), or None"""
    if min(in_dim, out_dim, z, g, w) < 1 or in_dim % w:
        return None
    Pin = in_dim // w
    if z > Pin:
        return None
    Q = 1 + (Pin - z) // g
    return (Pin, Q) if Q * w == out_dim else None


def pool_forward(x, geom):
    z, g, w = geom
    rows, Pin = x.shape[0], x.shape[1] // w
    Q = 1 + (Pin - z) // g
    xb = x.reshape(rows, Pin, w)
    out = np.empty((rows, Q, w), x.dtype)
    for q in range(Q):
        m = xb[:, q * g].copy()
        for j in range(1, z):
            v = xb[:, q * g + j]
            m = np.where(v > m, v, m)
        out[:, q] = m
    return out.reshape(rows, Q * w)


def pool_backward(x, out, out_diff, geom):
    """nnet1's rule: the equal-element mask over the pools that contain the patch, in order of q from +0, times 1 / c_p last"""
    z, g, w = geom
    rows, Pin = x.shape[0], x.shape[1] // w
    Q = 1 + (Pin - z) // g
    dt = x.dtype.type
    xb, ob, db = x.reshape(rows, Pin, w), out.reshape(rows, Q, w), out_diff.reshape(rows, Q, w)
    ind = np.zeros((rows, Pin, w), x.dtype)
    for p in range(Pin):
        qs = [q for q in range(Q) if q * g <= p < q * g + z]
        if not qs:
            continue
        s = np.zeros((rows, w), x.dtype)
        for q in qs:
            s = s + np.where(xb[:, p] == ob[:, q], db[:, q], dt(0))
        ind[:, p] = s * (dt(1) / dt(len(qs)))
    return ind.reshape(rows, Pin * w)


def activation(kind, x, dtype):
    x = x.astype(dtype)
    if kind == TANH:
        return np.tanh(x)
    with np.errstate(over="ignore"):
        return dtype(1) / (dtype(1) + np.exp(-x))


def activation_diff(kind, y, out_diff, dtype):
    y, d = y.astype(dtype), out_diff.astype(dtype)
    return d * (dtype(1) - y * y) if kind == TANH else d * y * (dtype(1) - y)


def rel_err(a, truth):
    """the project's measure: max|a - truth| / max|truth| per tensor"""
    return float(np.abs(a.astype(np.float64) - truth).max() / (np.abs(truth).max() + 1e-300))
