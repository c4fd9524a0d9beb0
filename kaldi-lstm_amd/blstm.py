"""BidirectionalLstm: the bidirectional LSTMP layer over whole utterances (include/klstm_blstm.hpp) on two Engines.

Plumbing only: the forward engine runs on `x`, the backward engine on klstm_reverse_streams' per-stream reversal of `x`, and the same
kernel puts the backward half of out back in time order, builds both halves of out_diff and adds the two halves of in_diff.  Padding
rows (t >= lens[s]) of out and in_diff come out zero; out_diff's padding rows are never read.  Both engines and every reversal run on
one stream (never two: the persistent chains would make each other give up), with "persist_verify" on, so that a persistent launch
that gives up is answered before a reversal reads its output."""
import numpy as np

from .binding import (Engine, REVERSE_ADD, REVERSE_MASK_COPY, REVERSE_SET, REVERSE_ZERO_PAD, BPTT_FUSE_UPDATE, reverse_streams)


class BidirectionalLstm:
    def __init__(self, input_dim, cell_dim, recur_dim, num_stream, device=0, stream=None):
        self.fwd = Engine(input_dim, cell_dim, recur_dim, num_stream, device, stream)
        self.bwd = Engine(input_dim, cell_dim, recur_dim, num_stream, device, stream)
        for e in (self.fwd, self.bwd):
            e.set_option("persist_verify", 1)
        self.I, self.C, self.R, self.S = input_dim, cell_dim, recur_dim, num_stream
        self.device, self.stream = device, stream
        self.T = 0
        self._buf = {}
        self._pending = None          # in_diff whose backward half is added in update() (BPTT_FUSE_UPDATE)

    def close(self):
        self.fwd.close()
        self.bwd.close()

    # ---- parameters: GetParams order per direction, forward block first ----
    @property
    def num_params(self):
        return self.fwd.num_params + self.bwd.num_params

    def set_params(self, fwd, bwd):
        self.fwd.set_params(fwd)
        self.bwd.set_params(bwd)

    def get_params(self):
        return np.concatenate([self.fwd.get_params(), self.bwd.get_params()])

    def get_corr(self):
        return np.concatenate([self.fwd.get_corr(), self.bwd.get_corr()])

    def _scratch(self, name, rows, cols):
        import torch
        t = self._buf.get(name)
        if t is None or t.shape != (rows, cols):
            t = torch.empty(rows, cols, device=f"cuda:{self.device}")
            self._buf[name] = t
        return t

    def _lens(self, lens, T):
        """lens: S lengths in [0, T] (host sequence, checked here) or an int32 CUDA tensor (clamped to [0, T] by the kernel)."""
        import torch
        if isinstance(lens, torch.Tensor) and lens.is_cuda:
            assert lens.dtype == torch.int32 and lens.numel() == self.S
            return lens.contiguous()
        h = np.asarray(lens, dtype=np.int64).ravel()
        if h.size != self.S or (h < 0).any() or (h > T).any():
            raise ValueError(f"lens must hold {self.S} lengths in [0, {T}], got {h.tolist()}")
        t = torch.tensor(h.astype(np.int32), device=f"cuda:{self.device}")
        if self.stream is not None:
            t.record_stream(self.stream)
        return t

    # ---- PropagateFnc / BackpropagateFnc / Update ----
    def propagate(self, x, lens, out):
        """x [T*S, I], out [T*S, 2R] (torch CUDA float32, last dim contiguous): columns [0, R) forward, [R, 2R) backward."""
        rows, R, S = x.shape[0], self.R, self.S
        assert rows % S == 0 and out.shape == (rows, 2 * R)
        T = rows // S
        self._ld = self._lens(lens, T)
        self.T = T
        self.fwd.reset([1] * S)
        self.bwd.reset([1] * S)
        xb, ob = self._scratch("xb", rows, self.I), self._scratch("ob", rows, R)
        self.fwd.propagate(x, out[:, :R])
        reverse_streams(x, self._ld, T, xb, REVERSE_SET, self.stream)
        self.bwd.propagate(xb, ob)
        reverse_streams(ob, self._ld, T, out[:, R:], REVERSE_SET, self.stream)
        reverse_streams(None, self._ld, T, out[:, :R], REVERSE_ZERO_PAD, self.stream)
        self._keep = [x, out]

    def backpropagate(self, x, out_diff, lens=None, in_diff=None, momentum=0.0, flags=0):
        """For the minibatch of the preceding propagate (same x; lens None = the same lengths).  out_diff [T*S, 2R]; in_diff [T*S, I] or
        None.  flags: the engines' (BPTT_FUSE_UPDATE: update() follows, and in_diff is complete when it has returned)."""
        rows, R, S, T = x.shape[0], self.R, self.S, self.T
        assert rows == T * S and out_diff.shape == (rows, 2 * R) and (in_diff is None or in_diff.shape == (rows, self.I))
        if lens is not None:
            self._ld = self._lens(lens, T)
        odf, odb = self._scratch("odf", rows, R), self._scratch("odb", rows, R)
        reverse_streams(out_diff[:, :R], self._ld, T, odf, REVERSE_MASK_COPY, self.stream)
        self.fwd.backpropagate(x, odf, in_diff, momentum, flags)
        reverse_streams(out_diff[:, R:], self._ld, T, odb, REVERSE_SET, self.stream)
        idb = self._scratch("idb", rows, self.I) if in_diff is not None else None
        self.bwd.backpropagate(self._buf["xb"], odb, idb, momentum, flags)
        self._pending = in_diff
        self._keep += [out_diff, in_diff]
        if not flags & BPTT_FUSE_UPDATE:
            self._combine()

    def _combine(self):
        ind, self._pending = self._pending, None
        if ind is None:
            return
        reverse_streams(self._buf["idb"], self._ld, self.T, ind, REVERSE_ADD, self.stream)
        reverse_streams(None, self._ld, self.T, ind, REVERSE_ZERO_PAD, self.stream)

    def update(self, learn_rate, clip_grad=0.0):
        self.fwd.update(learn_rate, clip_grad)
        self.bwd.update(learn_rate, clip_grad)
        self._combine()

    def synchronize(self):
        self.fwd.synchronize()
        self.bwd.synchronize()
