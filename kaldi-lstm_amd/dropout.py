"""Forward-connection dropout over the kdrop_* entries of include/klstm_dropout.h (which defines the mask: Philox4x32-10 over
(seed, salt, step, row or sequence, column); the numpy twin: tests/dropout_ref.py).  Plumbing only, no arithmetic: the numbers come
from kdrop_threshold and kdrop_apply, and without the library or a GPU the calls raise."""
import ctypes

from .binding import _chk, _sp, load_library

DROPOUT_ELEMENT, DROPOUT_SEQUENCE = 0, 1


def dropout_threshold(retention):
    """kdrop_threshold: (thr, scale) of a retention in [2^-32, 1] -- an element is kept iff its 32-bit word is below thr, and a kept
    element is multiplied by scale.  Host only.  Raises KlstmError outside the range."""
    thr, scale = ctypes.c_uint(0), ctypes.c_float(0)
    _chk(load_library().kdrop_threshold(float(retention), ctypes.byref(thr), ctypes.byref(scale)))
    return thr.value, scale.value


def dropout_apply(x, out, retention, seed, step, salt, mode=DROPOUT_ELEMENT, num_stream=1, seq_ids=None, stream=None):
    """kdrop_apply on torch CUDA float32 tensors [rows, cols] (row windows and column windows are fine; out may be x itself).
    seq_ids: with DROPOUT_SEQUENCE an int32 CUDA tensor of num_stream ids (read as unsigned).  The backward pass is the same call on
    out_diff with the same counters.  Asynchronous."""
    import torch
    assert x.is_cuda and out.is_cuda and x.dtype == torch.float32 and out.dtype == torch.float32 and x.dim() == 2 and x.shape == out.shape
    assert x.shape[1] == 0 or (x.stride(1) == 1 and out.stride(1) == 1)
    ids = None
    if mode == DROPOUT_SEQUENCE:
        assert seq_ids is not None and seq_ids.is_cuda and seq_ids.dtype == torch.int32 and seq_ids.is_contiguous() and seq_ids.numel() == num_stream
        ids = seq_ids.data_ptr()
    _chk(load_library().kdrop_apply(x.data_ptr(), x.stride(0), x.shape[0], x.shape[1], out.data_ptr(), out.stride(0), float(retention),
                                    int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFF, int(salt), int(mode), int(num_stream), ids,
                                    _sp(stream)))


class Dropout:
    """The <Dropout> component of include/klstm_nnet.hpp with the same counters: OFF until `training` is set; `step` advances with
    every active forward(); backward() replays the counters of the last forward(); with per_sequence a stream takes the next id of
    the layer's counter whenever reset(flags) flags it, and the ids go to the device only when they changed.  set_seed winds the
    counters back: the same seed and the same calls give the same masks bit for bit."""

    def __init__(self, retention, seed=0, salt=0, per_sequence=False):
        dropout_threshold(retention)                      # refuses a retention the kernel would refuse
        self.retention = float(retention)
        self.training = False
        self.per_sequence = bool(per_sequence)
        self.set_seed(seed, salt)

    def set_seed(self, seed, salt=None):
        self.seed = int(seed)
        if salt is not None:
            assert 0 <= int(salt) < 2 ** 31
            self.salt = int(salt)
        self.step = self._last_step = 0
        self._next_seq = 0
        self._seq_ids = []
        self._ids_dev = None

    def reset(self, flags):
        flags = [int(f) for f in flags]
        if len(flags) != len(self._seq_ids):              # a new stream count: every stream starts a sequence
            flags = [1] * len(flags)
            self._seq_ids = [0] * len(flags)
        for s, f in enumerate(flags):
            if f:
                self._seq_ids[s] = self._next_seq & 0xFFFFFFFF
                self._next_seq += 1
                self._ids_dev = None

    def _apply(self, x, out, stream):
        seq = self.training and self.per_sequence and self.retention != 1.0
        ids = None
        if seq:
            import torch
            if not self._seq_ids:
                raise RuntimeError("Dropout: per-sequence masks need a reset(flags) before the first forward")
            if self._ids_dev is None or self._ids_dev.device != x.device:
                self._ids_dev = torch.tensor(self._seq_ids, dtype=torch.int64).to(torch.int32).to(x.device)
            ids = self._ids_dev
        dropout_apply(x, out, self.retention if self.training else 1.0, self.seed, self._last_step, self.salt,
                      DROPOUT_SEQUENCE if seq else DROPOUT_ELEMENT, len(self._seq_ids) if seq else 1, ids, stream)
        return out

    def forward(self, x, out=None, stream=None):
        import torch
        if self.training:
            self._last_step = self.step
            self.step = (self.step + 1) & 0xFFFFFFFF
        return self._apply(x, torch.empty_like(x) if out is None else out, stream)

    def backward(self, out_diff, in_diff=None, stream=None):
        import torch
        return self._apply(out_diff, torch.empty_like(out_diff) if in_diff is None else in_diff, stream)
