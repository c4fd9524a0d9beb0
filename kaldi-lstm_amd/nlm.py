"""Rescoring of CTC n-best lists with an LSTM language model on the device (the knlm_* entries of include/klstm_nlm.h, which defines
every quantity) on torch CUDA tensors.  Plumbing only: CtcNeuralLm holds the engines and the device
copies of the Affine parameters and runs the plan -- per group of entries and chunk of positions knlm_pack -> propagate_inference per
layer -> affine_propagate -> knlm_score_rows, then one knlm_rank -- with nothing read back.  knlm_pack, knlm_score_rows and knlm_rank
are the entries themselves; lm_training_utterances makes the training data of such a model."""
import collections
import ctypes

import numpy as np

from .binding import Engine, _chk, _sp, affine_propagate, load_library
from .ctc import CtcBeamResult, _check_totals, _nbest_arrays, _ptr

# order [S, N] int32 (the entry of rank r; -1 beyond live_count), live_count [S], score [S, N] float32 (float(z); -inf: dropped, forbidden
# or unlisted), nlm_logp [S, N] float32 (-inf likewise), units [S, N] int32, nbest: the re-ranked list as a CtcBeamResult (None with
# out_n = 0), acc [S, N] float64 and positions [S, N] int32: what knlm_score_rows accumulated (None from knlm_rank alone)
CtcNeuralRescoreResult = collections.namedtuple("CtcNeuralRescoreResult", "order live_count score nlm_logp units nbest acc positions")


def _lists(nbest, logp=None, max_len=None):
    hyp, hyp_len, count, errors, logp, S, N, stride = _nbest_arrays(nbest, logp)
    max_len = min(1023, stride) if max_len is None else int(max_len)
    return hyp, hyp_len, count, errors, logp, S, N, max(stride, 1), max_len


def knlm_workspace_bytes(E, T):
    n = load_library().knlm_workspace_bytes(int(E), int(T))
    if n == 0:
        _chk(2)
    return n


def knlm_pack(nbest, K, V, bos, eos, first_entry, E, T, t0, out, embed=None, logp=None, max_len=None, stream=None):
    """knlm_pack: the engine input of positions t0 .. t0 + T - 1 of the entries first_entry .. first_entry + E - 1 into out [T * E, >= V]
    (one-hot rows) or, with embed = (W [D, V], bias [D]) CUDA tensors, [T * E, >= D] (columns of W plus the bias).  nbest, logp: as
    ctc_nbest_rescore takes them."""
    hyp, hyp_len, count, _, logp, S, N, stride, max_len = _lists(nbest, logp, max_len)
    W, bias = embed if embed is not None else (None, None)
    assert out.is_cuda and out.stride(1) == 1 and out.shape[0] == T * E
    assert W is None or (W.is_contiguous() and bias.is_contiguous() and W.shape[1] == V and bias.numel() == W.shape[0])
    _chk(load_library().knlm_pack(hyp.data_ptr(), stride, hyp_len.data_ptr(), count.data_ptr(), logp.data_ptr(), S, N, max_len, int(K), int(V),
                                  int(bos), int(eos), int(first_entry), int(E), int(T), int(t0), _ptr(W), _ptr(bias),
                                  W.shape[0] if W is not None else 0, out.data_ptr(), out.stride(0), _sp(stream)))


def knlm_score_rows(a, nbest, K, eos, first_entry, E, T, t0, acc, positions=None, logp=None, max_len=None, workspace=None, stream=None):
    """knlm_score_rows: a [T * E, V] float32, the rows of the last Affine for the chunk knlm_pack made with the same arguments; acc [S, N]
    float64 and positions [S, N] int32 (or None) are set by the chunk with t0 == 0 and added to by the later ones."""
    import torch
    hyp, hyp_len, count, _, logp, S, N, stride, max_len = _lists(nbest, logp, max_len)
    assert a.is_cuda and a.dtype == torch.float32 and a.stride(1) == 1 and a.shape[0] == T * E
    assert acc.dtype == torch.float64 and acc.numel() == S * N and acc.is_contiguous()
    assert positions is None or (positions.dtype == torch.int32 and positions.numel() == S * N and positions.is_contiguous())
    nbytes = knlm_workspace_bytes(E, T)
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=a.device)
    _chk(load_library().knlm_score_rows(a.data_ptr(), a.stride(0), hyp.data_ptr(), stride, hyp_len.data_ptr(), count.data_ptr(), logp.data_ptr(),
                                        S, N, max_len, int(K), a.shape[1], int(eos), int(first_entry), int(E), int(T), int(t0), acc.data_ptr(),
                                        _ptr(positions), workspace.data_ptr(), ctypes.c_size_t(workspace.numel()), _sp(stream)))


def knlm_rank(nbest, K, acc, has_eos, am_scale=1.0, nlm_scale=1.0, unit_bonus=0.0, out_n=None, logp=None, max_len=None, out_stride=None,
              out=None, totals=None, positions=None, stream=None):
    """knlm_rank: z = am_scale * logp + nlm_scale * acc + unit_bonus * units, the ranking and the re-ranked list.  out: a CtcBeamResult to
    gather into (None: a fresh one, zeros / -inf / -1 beyond the counts); totals: a float64[8] CUDA tensor the minibatch is added to.
    stream: a torch stream to launch on; it is made to wait for the caller's current stream first, on which the outputs are created, and
    the caller orders what reads the result behind it (CtcNeuralLm.rescore does).  -> CtcNeuralRescoreResult"""
    import torch
    hyp, hyp_len, count, errors, logp, S, N, stride, max_len = _lists(nbest, logp, max_len)
    dev = hyp.device
    assert acc.dtype == torch.float64 and acc.numel() == S * N and acc.is_contiguous()
    out_n = N if out_n is None else int(out_n)
    _check_totals(totals, 8)
    order = torch.empty(S, N, dtype=torch.int32, device=dev)
    live = torch.empty(S, dtype=torch.int32, device=dev)
    score, nlm_logp = (torch.empty(S, N, device=dev) for _ in range(2))
    units = torch.empty(S, N, dtype=torch.int32, device=dev)
    if out_n >= 1 and out is None:
        out_stride = max(min(stride, max_len), 1) if out_stride is None else int(out_stride)
        out = CtcBeamResult(torch.zeros(S, out_n, out_stride, dtype=torch.int32, device=dev), torch.zeros(S, out_n, dtype=torch.int32, device=dev),
                            torch.zeros(S, dtype=torch.int32, device=dev), torch.full((S, out_n), -np.inf, device=dev),
                            torch.full((S, out_n), -1, dtype=torch.int32, device=dev) if errors is not None else None)
    if out_n < 1:
        out = None
    if stream is not None:                                 # the outputs above were created and filled on the caller's current stream
        stream.wait_stream(torch.cuda.current_stream())
    _chk(load_library().knlm_rank(hyp.data_ptr(), stride, hyp_len.data_ptr(), count.data_ptr(), logp.data_ptr(), _ptr(errors), S, N, max_len, int(K),
                                  acc.data_ptr(), float(am_scale), float(nlm_scale), float(unit_bonus), 1 if has_eos else 0, order.data_ptr(),
                                  live.data_ptr(), score.data_ptr(), nlm_logp.data_ptr(), units.data_ptr(), out_n, _ptr(out.hyp) if out else None,
                                  out.hyp.stride(1) if out else 0, _ptr(out.hyp_len) if out else None, _ptr(out.nbest_count) if out else None,
                                  _ptr(out.score) if out else None, _ptr(out.errors) if out else None, _ptr(totals), _sp(stream)))
    return CtcNeuralRescoreResult(order, live, score, nlm_logp, units, out, acc.view(S, N), positions.view(S, N) if positions is not None else None)


class CtcNeuralLm:
    """An LSTM language model over the tokens of a CTC model, for the second pass over its n-best lists.  layers: a list of (flat
    LstmProjectedStreams parameters, input dim, cell dim, recurrent dim); W [V, R], b [V]: the last Affine (a Softmax behind it is folded
    into the scoring); embed: None (one-hot input: the first layer's input dim is V) or (We [D, V], be [D]), an embedding Affine (the
    first layer's input dim is D).  V classes, of which 0 .. classes - 1 (default: all V) are the CTC model's tokens; bos, eos: classes
    (eos < 0: no end term; bos = eos = blank with V = K is the economical choice).  num_stream entries are scored at a time, in chunks of
    `chunk` positions.  stream: None (the engines' shared stream and the default stream, ordered with each other as the library's other
    calls are), or a torch stream that the engines and every launch of the pass are put on; the pass is then ordered behind the caller's
    current stream at its start and in front of it at its end.  Owns its engines (close() frees them)."""

    def __init__(self, layers, W, b, embed=None, bos=0, eos=0, num_stream=16, chunk=20, classes=None, device=0, stream=None):
        import torch
        W, b = np.ascontiguousarray(W, np.float32), np.ascontiguousarray(b, np.float32)
        self.V, self.E, self.T, self.bos, self.eos = int(W.shape[0]), int(num_stream), int(chunk), int(bos), int(eos)
        self.K = self.V if classes is None else int(classes)
        dev = torch.device("cuda", device)
        self.device, self.stream = dev, stream
        self.cols = self.V if embed is None else int(np.asarray(embed[0]).shape[0])
        dims = [(int(i), int(c), int(r)) for _, i, c, r in layers]
        if not dims or dims[0][0] != self.cols or any(dims[l][0] != dims[l - 1][2] for l in range(1, len(dims))) or W.shape != (self.V, dims[-1][2]) \
                or b.shape != (self.V,) or not 0 <= self.bos < self.V or self.eos >= self.V or not 2 <= self.K <= self.V:
            raise ValueError("CtcNeuralLm: [embedding D x V] -> LSTM layers (V or D -> R, R -> R, ...) -> Affine V x R, bos and eos classes in [0, V)")
        self.engines = []
        for (flat, _, _, _), (i, c, r) in zip(layers, dims):
            e = Engine(i, c, r, self.E, device=device, stream=stream)
            e.set_params(flat)
            e.set_option("persist_verify", 1)              # a persistent launch that gives up is run again inside its call: the buffers are reused
            self.engines.append(e)
        self.W, self.b = torch.from_numpy(W).to(dev), torch.from_numpy(b).to(dev)
        self.embed = None
        if embed is not None:
            We, be = np.ascontiguousarray(embed[0], np.float32), np.ascontiguousarray(embed[1], np.float32)
            assert We.shape == (self.cols, self.V) and be.shape == (self.cols,)
            self.embed = (torch.from_numpy(We).to(dev), torch.from_numpy(be).to(dev))
        rows = self.T * self.E
        self.x = torch.empty(rows, self.cols, device=dev)
        self.h = [torch.empty(rows, r, device=dev) for _, _, r in dims]
        self.a = torch.empty(rows, self.V, device=dev)
        self.ws = torch.empty(knlm_workspace_bytes(self.E, self.T), dtype=torch.uint8, device=dev)

    def close(self):
        for e in self.engines:
            e.close()
        self.engines = []

    def accumulate(self, nbest, logp=None, max_len=None):
        """the scoring loop alone -> (acc [S, N] float64, positions [S, N] int32).  Nothing synchronises."""
        import torch
        hyp, hyp_len, count, _, logp, S, N, stride, max_len = _lists(nbest, logp, max_len)
        assert hyp.device == self.device, "the lists live on the model's device"
        lists = (hyp, hyp_len, count, None)
        acc = torch.zeros(S, N, dtype=torch.float64, device=self.device)
        pos = torch.zeros(S, N, dtype=torch.int32, device=self.device)
        E, T = self.E, self.T
        chunks = (max_len + (1 if self.eos >= 0 else 0) + T - 1) // T
        ones = np.ones(E, np.int32)
        st = self.stream
        if st is not None:
            st.wait_stream(torch.cuda.current_stream())
        for first in range(0, S * N, E):
            for e in self.engines:
                e.reset(ones)
            for c in range(chunks):
                knlm_pack(lists, self.K, self.V, self.bos, self.eos, first, E, T, c * T, self.x, self.embed, logp, max_len, st)
                h = self.x
                for l, e in enumerate(self.engines):
                    e.propagate_inference(h, self.h[l])
                    h = self.h[l]
                affine_propagate(h, self.W, self.b, self.a, st)
                knlm_score_rows(self.a, lists, self.K, self.eos, first, E, T, c * T, acc, pos, logp, max_len, self.ws, st)
        if st is not None:
            torch.cuda.current_stream().wait_stream(st)
        return acc, pos

    def rescore(self, nbest, am_scale=1.0, nlm_scale=1.0, unit_bonus=0.0, out_n=None, logp=None, max_len=None, totals=None):
        """nbest: the CtcBeamResult of ctc_beam_decode, the dict of ctc_nbest_rescore (its re-ranked list), or a tuple of arrays with logp,
        as ctc_nbest_rescore takes them.  z = am_scale * logp + nlm_scale * nlm_logp + unit_bonus * units -> CtcNeuralRescoreResult, which
        ctc_nbest_consensus, ctc_mbr_eval and nbest_to_lists take in place of the search's result.  max_len: the token capacity the plan is
        laid out for (None: min(1023, the lists' stride)); totals: a float64[8] CUDA tensor.  Nothing synchronises."""
        import torch
        acc, pos = self.accumulate(nbest, logp, max_len)
        r = knlm_rank(nbest, self.K, acc, self.eos >= 0, am_scale, nlm_scale, unit_bonus, out_n, logp, max_len, totals=totals, positions=pos,
                      stream=self.stream)
        if self.stream is not None:
            torch.cuda.current_stream().wait_stream(self.stream)
        return r

    def score(self, nbest, logp=None, max_len=None):
        """-> nlm_logp [S, N] float32 (-inf: dropped, forbidden or unlisted)"""
        return self.rescore(nbest, logp=logp, max_len=max_len, out_n=0).nlm_logp


def lm_training_utterances(sequences, V, bos, eos):
    """Token sequences -> the training data of a token LM as (features, targets) pairs: features float32 [n, V], the one-hot rows of
    [bos, y_0, ...]; targets int32 [n], the next tokens [y_0, ..., eos].  With an end term (eos >= 0) n = len(y) + 1, without n = len(y)
    (a sequence that leaves no row is skipped)."""
    out = []
    for y in sequences:
        y = [int(t) for t in y]
        if any(t < 0 or t >= V for t in y) or not 0 <= bos < V or eos >= V:
            raise ValueError("lm_training_utterances: a class outside [0, %d)" % V)
        x, tgt = ([bos] + y, y + [eos]) if eos >= 0 else (([bos] + y)[:len(y)], y)
        if not x:
            continue
        feats = np.zeros((len(x), V), np.float32)
        feats[np.arange(len(x)), x] = 1
        out.append((feats, np.asarray(tgt, np.int32)))
    return out
