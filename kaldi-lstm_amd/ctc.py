"""ctc_eval: connectionist temporal classification over whole utterances (klstm_ctc_eval of include/klstm.h) on torch
CUDA tensors.  Plumbing only: the label lists become the CSR arrays of the C-ABI, the workspace is cached per shape.
ctc_greedy_decode: best-path decoding and token error rate of the same posteriors (klstm_ctc_decode).
ctc_align: the most probable alignment of given label sequences to the frames (klstm_ctc_align).
ctc_beam_decode: prefix beam search, n-best lists with scores and edit distances (klstm_ctc_beam_decode), with
lm=CtcLabelLm(...) fused with a label language model or a lexicon (klstm_ctc_beam_decode_lm; tables: lm.py), or
lm=CtcSparseLabelLm(...) with a sparse back-off n-gram, read from an ARPA file or counted (klstm_ctc_beam_decode_slm).
CtcBeamStream: the same search fed chunk by chunk, the beam kept on the device between the calls (klstm_ctc_beam_stream_step / _emit;
INTEGRATION.md 3j).
ctc_mbr_eval: the expected token errors over such n-best lists and their gradient (klstm_ctc_mbr_eval).
ctc_nbest_consensus: MBR decoding and token / word confidences over such n-best lists (klstm_ctc_consensus).
ctc_nbest_rescore: such lists re-ranked with token and word back-off models, between the two (klstm_ctc_nbest_rescore).
CtcMmiDenominator / ctc_mmi_eval: MMI (CTC-CRF) against the language model the beam search uses (klstm_ctc_mmi_eval)."""
import collections
import ctypes

import numpy as np

from .binding import _chk, _sp, load_library
from .lm import split_words

_WS = {}          # operation -> {(device, the shape its workspace depends on) -> uint8 workspace tensor}


def _workspace_bytes(fn_name, *args):
    n = getattr(load_library(), fn_name)(*(int(a) for a in args))
    if n == 0:
        _chk(2)
    return n


def _workspace(op, key, nbytes, dev):
    """the cached workspace of operation `op` for the shape `key`; an operation that has seen 8 shapes starts over"""
    import torch
    cache = _WS.setdefault(op, {})
    key = (dev.index,) + tuple(key)
    ws = cache.get(key)
    if ws is None:
        if len(cache) >= 8:
            cache.clear()
        ws = cache[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return ws


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _shape(net_out, lens):
    """(net_out [T*S, K], lens) -> (lens as an int32 tensor on net_out's device, S, T, K)"""
    import torch
    assert net_out.is_cuda and net_out.dtype == torch.float32 and net_out.dim() == 2 and net_out.stride(1) == 1
    if isinstance(lens, torch.Tensor) and lens.is_cuda:
        assert lens.dtype == torch.int32 and lens.is_contiguous()
        lens_dev = lens
    else:
        lens_dev = torch.tensor([int(v) for v in lens], dtype=torch.int32, device=net_out.device)
    S = lens_dev.numel()
    assert S > 0 and net_out.shape[0] % S == 0, "rows must be T * len(lens)"
    return lens_dev, S, net_out.shape[0] // S, net_out.shape[1]


def _check_class_weight(class_weight, K):
    import torch
    if class_weight is not None:
        assert class_weight.is_cuda and class_weight.dtype == torch.float32 and class_weight.numel() == K and class_weight.is_contiguous()


def _check_totals(totals, n):
    import torch
    if totals is not None:
        assert totals.is_cuda and totals.dtype == torch.float64 and totals.numel() == n and totals.is_contiguous()


def _packed(labels, S, dev):
    """label lists, or what pack_labels() returned -> (labels, offsets, longest) on the device, checked against S streams"""
    import torch
    lab_dev, off_dev, longest = labels if isinstance(labels, tuple) else pack_labels(labels, dev)
    assert off_dev.numel() == S + 1 and lab_dev.dtype == torch.int32 and off_dev.dtype == torch.int32
    return lab_dev, off_dev, longest


def ctc_workspace_bytes(T, S, max_label_len):
    return _workspace_bytes("klstm_ctc_workspace_bytes", T, S, max_label_len)


def pack_labels(labels, device):
    """list of S label sequences -> (labels int32 [max(1, total)], offsets int32 [S+1], longest) on `device`"""
    import torch
    off = np.zeros(len(labels) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(lab) for lab in labels])
    flat = np.concatenate([np.asarray(lab, dtype=np.int32).ravel() for lab in labels] + [np.zeros(0, np.int32)])
    if flat.size == 0:
        flat = np.zeros(1, np.int32)
    longest = max([len(lab) for lab in labels] + [0])
    return torch.from_numpy(flat).to(device), torch.from_numpy(off).to(device), longest


def ctc_eval(net_out, lens, labels, blank=0, diff=None, totals=None, stream=None):
    """net_out [T*S, K] float32 CUDA posteriors (row t*S + s; a column window with a larger row stride is fine); lens: S lengths (a
    sequence, or an int32 CUDA tensor); labels: a list of S label sequences, or what pack_labels() returned (a caller that keeps
    the arrays on the device).  Returns (utt_loss [S] float32, diff [T*S, K]): diff = y - gamma, the gradient with respect to the
    softmax input, zero on padding rows and on every row of an idle or rejected stream; utt_loss = -log p(labels | x), +inf for a
    rejected stream, 0 for an idle one.  totals: a float64[4] CUDA tensor that loss sum, utterances counted, utterances rejected
    and frames are added to.  Nothing synchronises."""
    import torch
    lib = load_library()
    dev = net_out.device
    lens_dev, S, T, K = _shape(net_out, lens)
    lab_dev, off_dev, longest = _packed(labels, S, dev)
    if diff is None:
        diff = torch.empty(T * S, K, device=dev)
    assert diff.is_cuda and diff.dtype == torch.float32 and diff.shape == (T * S, K) and diff.stride(1) == 1
    nbytes = ctc_workspace_bytes(T, S, longest)
    ws = _workspace("eval", (T, S, longest), nbytes, dev)
    utt_loss = torch.empty(S, device=dev)
    _check_totals(totals, 4)
    _chk(lib.klstm_ctc_eval(net_out.data_ptr(), T, S, K, net_out.stride(0), lens_dev.data_ptr(), lab_dev.data_ptr(), off_dev.data_ptr(),
                            int(blank), diff.data_ptr(), diff.stride(0), utt_loss.data_ptr(), _ptr(totals), ws.data_ptr(),
                            ctypes.c_size_t(nbytes), _sp(stream)))
    return utt_loss, diff


CtcDecodeResult = collections.namedtuple("CtcDecodeResult", "hyp hyp_len score frame_class errors")


def ctc_decode_workspace_bytes(T, S, max_ref_len=0):
    return _workspace_bytes("klstm_ctc_decode_workspace_bytes", T, S, max_ref_len)


def ctc_greedy_decode(net_out, lens, blank=0, class_weight=None, refs=None, totals=None, stream=None):
    """net_out [T*S, K] float32 CUDA posteriors (row t*S + s; a column window with a larger row stride is fine); lens: S lengths (a
    sequence, or an int32 CUDA tensor); class_weight: None or K float32 on the device (frame winner = argmax_k y[k] * w[k], one fp32
    product; label priors go in as prior ** -alpha); refs: None, a list of S reference label sequences, or what pack_labels()
    returned.  Returns CtcDecodeResult(hyp [S, T] int32 (row s valid up to hyp_len[s]), hyp_len [S] int32, score [S] float32,
    frame_class [T*S] int32 (-1 on padding and idle rows), errors [S] int32 edit distances (-1: not counted) or None without refs).
    totals: a float64[5] CUDA tensor that edit errors, reference tokens, hypothesis tokens, utterances counted and utterances with an
    error are added to (needs refs).  Nothing synchronises; hypotheses_to_lists() does."""
    import torch
    lib = load_library()
    dev = net_out.device
    lens_dev, S, T, K = _shape(net_out, lens)
    _check_class_weight(class_weight, K)
    lab_dev = off_dev = errors = None
    longest = 0
    if refs is not None:
        lab_dev, off_dev, longest = _packed(refs, S, dev)
        errors = torch.empty(S, dtype=torch.int32, device=dev)
    assert totals is None or refs is not None, "totals need refs"
    _check_totals(totals, 5)
    nbytes = ctc_decode_workspace_bytes(T, S, min(longest, 1023))       # a longer reference is the device's to refuse (errors -1)
    ws = _workspace("decode", (T, S), nbytes, dev)
    hyp = torch.empty(S, T, dtype=torch.int32, device=dev)
    hyp_len = torch.empty(S, dtype=torch.int32, device=dev)
    score = torch.empty(S, device=dev)
    frame_class = torch.empty(T * S, dtype=torch.int32, device=dev)
    _chk(lib.klstm_ctc_decode(net_out.data_ptr(), T, S, K, net_out.stride(0), lens_dev.data_ptr(), int(blank), _ptr(class_weight),
                              hyp.data_ptr(), hyp_len.data_ptr(), score.data_ptr(), frame_class.data_ptr(), _ptr(lab_dev), _ptr(off_dev),
                              _ptr(errors), _ptr(totals), ws.data_ptr(), ctypes.c_size_t(nbytes), _sp(stream)))
    return CtcDecodeResult(hyp, hyp_len, score, frame_class, errors)


def hypotheses_to_lists(hyp, hyp_len):
    """(hyp [S, T], hyp_len [S]) of ctc_greedy_decode -> S Python lists.  The one place that synchronises."""
    h, n = hyp.cpu().numpy(), hyp_len.cpu().numpy()
    return [h[s, :n[s]].tolist() for s in range(len(n))]


CtcAlignResult = collections.namedtuple("CtcAlignResult", "frame_class frame_pos token_begin token_end score")


def ctc_align_workspace_bytes(T, S, max_label_len):
    return _workspace_bytes("klstm_ctc_align_workspace_bytes", T, S, max_label_len)


def ctc_align(net_out, lens, labels, blank=0, class_weight=None, totals=None, stream=None):
    """The most probable alignment of labels[s] to the frames of stream s (Viterbi over the CTC lattice; ties: stay, advance, skip).
    net_out, lens, labels as ctc_eval takes them; class_weight: None or K float32 on the device (emission log(y[k] * w[k]), one fp32
    product; the score stays unweighted).  Returns CtcAlignResult(frame_class [T*S] int32 (the class of every frame on the path, -1
    on padding rows and on idle / rejected streams), frame_pos [T*S] int32 (label position of the frame, -1 on blank frames),
    token_begin, token_end (parallel to the packed labels: first frame of a token and one past its last; -1 where not aligned),
    score [S] float32 (0 idle, -inf rejected)).  totals: a float64[5] CUDA tensor that score sum, utterances aligned, utterances
    rejected, frames and blank frames are added to.  Nothing synchronises; alignments_to_lists() does."""
    import torch
    lib = load_library()
    dev = net_out.device
    lens_dev, S, T, K = _shape(net_out, lens)
    lab_dev, off_dev, longest = _packed(labels, S, dev)
    _check_class_weight(class_weight, K)
    _check_totals(totals, 5)
    cap = min(longest, 1023)                                            # a longer sequence is the device's to reject
    nbytes = ctc_align_workspace_bytes(T, S, cap)
    ws = _workspace("align", (T, S, cap), nbytes, dev)
    frame_class = torch.empty(T * S, dtype=torch.int32, device=dev)
    frame_pos = torch.empty(T * S, dtype=torch.int32, device=dev)
    token_begin = torch.empty(lab_dev.numel(), dtype=torch.int32, device=dev)
    token_end = torch.empty(lab_dev.numel(), dtype=torch.int32, device=dev)
    score = torch.empty(S, device=dev)
    _chk(lib.klstm_ctc_align(net_out.data_ptr(), T, S, K, net_out.stride(0), lens_dev.data_ptr(), lab_dev.data_ptr(), off_dev.data_ptr(),
                             int(blank), _ptr(class_weight), frame_class.data_ptr(), frame_pos.data_ptr(), token_begin.data_ptr(),
                             token_end.data_ptr(), score.data_ptr(), _ptr(totals), ws.data_ptr(), ctypes.c_size_t(nbytes), _sp(stream)))
    return CtcAlignResult(frame_class, frame_pos, token_begin, token_end, score)


def alignments_to_lists(result, lens, offsets):
    """CtcAlignResult -> per stream dict(frame_class, frame_pos (lists over the stream's frames), token_begin, token_end (lists over
    its labels), score); lens: S lengths, offsets: the S + 1 label offsets (a sequence or a tensor).  An idle or rejected stream
    (frame_class -1 throughout) gives empty frame lists.  The one place that synchronises."""
    lens = [int(v) for v in (lens.cpu().tolist() if hasattr(lens, "cpu") else lens)]
    off = [int(v) for v in (offsets.cpu().tolist() if hasattr(offsets, "cpu") else offsets)]
    S = len(lens)
    fc, fp = result.frame_class.cpu().numpy().reshape(-1, S), result.frame_pos.cpu().numpy().reshape(-1, S)
    tb, te, sc = result.token_begin.cpu().numpy(), result.token_end.cpu().numpy(), result.score.cpu().numpy()
    out = []
    for s in range(S):
        n = lens[s] if 0 < lens[s] <= fc.shape[0] and fc[0, s] >= 0 else 0
        out.append(dict(frame_class=fc[:n, s].tolist(), frame_pos=fp[:n, s].tolist(), token_begin=tb[off[s]:off[s + 1]].tolist(),
                        token_end=te[off[s]:off[s + 1]].tolist(), score=float(sc[s])))
    return out


CtcBeamResult = collections.namedtuple("CtcBeamResult", "hyp hyp_len nbest_count score errors")


def ctc_beam_workspace_bytes(T, S, beam, cands):
    return _workspace_bytes("klstm_ctc_beam_workspace_bytes", T, S, beam, cands)


class CtcLabelLm:
    """The device tables of a label language model for ctc_beam_decode(lm=...): a dense deterministic weighted automaton, next [Q, K]
    int32, weight [Q, K] float32, final [Q] float32 or None (klstm_ctc_beam_decode_lm of include/klstm.h).  Takes numpy arrays or
    tensors (ngram_label_lm / lexicon_label_lm of lm.py build them) and keeps contiguous copies on `device`."""

    def __init__(self, next, weight, final=None, device="cuda"):
        import torch

        def dev(a, dtype):
            return torch.as_tensor(a).to(device=device, dtype=dtype).contiguous()
        self.next, self.weight = dev(next, torch.int32), dev(weight, torch.float32)
        self.final = dev(final, torch.float32) if final is not None else None
        assert self.next.dim() == 2 and self.next.shape == self.weight.shape and self.next.shape[0] >= 1
        self.states, self.classes = int(self.next.shape[0]), int(self.next.shape[1])
        assert self.final is None or self.final.shape == (self.states,)

    def resident(self, beam, cands):
        """whether a call of this shape looks the tables up in LDS (True) or gathers them from global memory"""
        return bool(load_library().klstm_ctc_beam_lm_resident(self.states, self.classes, int(beam), int(cands)))


class CtcSparseLabelLm:
    """A sparse back-off language model on the device for ctc_beam_decode(lm=...) and CtcBeamStream(lm=...): the arrays of a
    lm.SparseLm (arpa_label_lm / backoff_ngram_label_lm build them) turned into the blob the search walks (klstm_ctc_slm_build of
    include/klstm.h), once.  The build validates on the device: `status` (a CUDA int32[8]; status_list() synchronises) counts the
    states it dropped and the back-offs it cut.  final: the model's own unless given; None in the model: no final weights."""

    def __init__(self, model, blank, final="model", device="cuda", stream=None):
        import torch

        def dev(a, dtype):
            return torch.as_tensor(np.asarray(a)).to(device=device, dtype=dtype).contiguous()
        lib = load_library()
        self.classes, self.blank = int(model.classes), int(blank)
        self.states, self.arcs = len(model.backoff), len(model.arc_labels)
        off, lab, nxt = dev(model.arc_offsets, torch.int32), dev(model.arc_labels, torch.int32), dev(model.arc_next, torch.int32)
        wt, bo, bow = dev(model.arc_weight, torch.float32), dev(model.backoff, torch.int32), dev(model.backoff_weight, torch.float32)
        assert off.numel() == self.states + 1 and nxt.numel() == self.arcs and wt.numel() == self.arcs and bow.numel() == self.states
        final = model.final if isinstance(final, str) else final
        self.final = dev(final, torch.float32) if final is not None else None
        assert self.final is None or self.final.shape == (self.states,)
        self.nbytes = _workspace_bytes("klstm_ctc_slm_bytes", self.states, self.arcs, self.classes)
        self.blob = torch.empty(self.nbytes, dtype=torch.uint8, device=device)
        self.status = torch.zeros(8, dtype=torch.int32, device=device)
        _chk(lib.klstm_ctc_slm_build(self.states, self.arcs, self.classes, self.blank, off.data_ptr(), lab.data_ptr(), nxt.data_ptr(),
                                     wt.data_ptr(), bo.data_ptr(), bow.data_ptr(), self.blob.data_ptr(), ctypes.c_size_t(self.nbytes),
                                     self.status.data_ptr(), _sp(stream)))
        self._inputs = (off, lab, nxt, wt, bo, bow)                      # alive until the build has run

    @property
    def device(self):
        return self.blob.device

    def status_list(self):
        return self.status.cpu().tolist()


def _lm_device(lm):
    return lm.blob.device if isinstance(lm, CtcSparseLabelLm) else lm.next.device


def ctc_beam_decode(net_out, lens, blank=0, beam=16, cands=8, nbest=1, class_weight=None, refs=None, totals=None, stream=None, lm=None):
    """CTC prefix beam search: the most probable LABELLINGS of every stream, best first.  net_out, lens, class_weight and refs as
    ctc_greedy_decode takes them; beam <= 64 prefixes survive a frame, each extended by the cands <= min(K - 1, 32) best classes of
    the frame, nbest <= beam of them are returned.  Returns CtcBeamResult(hyp [S, N, T] int32 (row (s, q) valid up to hyp_len[s, q]),
    hyp_len [S, N] int32, nbest_count [S] int32 (list slots beyond it are not written), score [S, N] float32 (log probability as the
    search summed it), errors [S, N] int32 edit distances (-1: not counted, or no such slot) or None without refs).  totals: a
    float64[6] CUDA tensor that 1-best edit errors, reference tokens, 1-best hypothesis tokens, utterances counted, utterances with a
    1-best error and oracle errors (the minimum over the list) are added to (needs refs).  lm: a CtcLabelLm or a CtcSparseLabelLm whose factors enter
    every extension; the scores are then the fused ones, acoustic times language model.  Nothing synchronises; nbest_to_lists()
    does."""
    import torch
    lib = load_library()
    dev = net_out.device
    lens_dev, S, T, K = _shape(net_out, lens)
    beam, cands, nbest = int(beam), int(cands), int(nbest)
    _check_class_weight(class_weight, K)
    lab_dev = off_dev = errors = None
    if refs is not None:
        lab_dev, off_dev, _ = _packed(refs, S, dev)
    assert totals is None or refs is not None, "totals need refs"
    _check_totals(totals, 6)
    nbytes = ctc_beam_workspace_bytes(T, S, beam, cands)
    ws = _workspace("beam", (T, S, beam, cands), nbytes, dev)
    hyp = torch.empty(S, max(nbest, 0), T, dtype=torch.int32, device=dev)
    hyp_len = torch.empty(S, max(nbest, 0), dtype=torch.int32, device=dev)
    count = torch.empty(S, dtype=torch.int32, device=dev)
    score = torch.empty(S, max(nbest, 0), device=dev)
    if refs is not None:
        errors = torch.empty(S, max(nbest, 0), dtype=torch.int32, device=dev)
    if lm is None:
        _chk(lib.klstm_ctc_beam_decode(net_out.data_ptr(), T, S, K, net_out.stride(0), lens_dev.data_ptr(), int(blank), _ptr(class_weight),
                                       beam, cands, nbest, hyp.data_ptr(), hyp_len.data_ptr(), count.data_ptr(), score.data_ptr(),
                                       _ptr(lab_dev), _ptr(off_dev), _ptr(errors), _ptr(totals), ws.data_ptr(), ctypes.c_size_t(nbytes), _sp(stream)))
    elif isinstance(lm, CtcSparseLabelLm):
        assert lm.classes == K and lm.blob.device == dev, "the language model has K classes and lives on net_out's device"
        _chk(lib.klstm_ctc_beam_decode_slm(net_out.data_ptr(), T, S, K, net_out.stride(0), lens_dev.data_ptr(), int(blank), _ptr(class_weight),
                                           beam, cands, nbest, lm.blob.data_ptr(), ctypes.c_size_t(lm.nbytes), lm.states, _ptr(lm.final),
                                           hyp.data_ptr(), hyp_len.data_ptr(), count.data_ptr(), score.data_ptr(), _ptr(lab_dev), _ptr(off_dev),
                                           _ptr(errors), _ptr(totals), ws.data_ptr(), ctypes.c_size_t(nbytes), _sp(stream)))
    else:
        assert lm.classes == K and lm.next.device == dev, "the language model's tables have K columns and live on net_out's device"
        _chk(lib.klstm_ctc_beam_decode_lm(net_out.data_ptr(), T, S, K, net_out.stride(0), lens_dev.data_ptr(), int(blank), _ptr(class_weight),
                                          beam, cands, nbest, lm.states, lm.next.data_ptr(), lm.weight.data_ptr(), _ptr(lm.final),
                                          hyp.data_ptr(), hyp_len.data_ptr(), count.data_ptr(), score.data_ptr(), _ptr(lab_dev), _ptr(off_dev),
                                          _ptr(errors), _ptr(totals), ws.data_ptr(), ctypes.c_size_t(nbytes), _sp(stream)))
    return CtcBeamResult(hyp, hyp_len, count, score, errors)


def _as_nbest(nbest):
    """what ctc_nbest_rescore (a dict) or CtcNeuralLm.rescore (nlm.CtcNeuralRescoreResult) returned stands for its re-ranked list"""
    if isinstance(nbest, dict):
        assert nbest.get("nbest") is not None, "the rescoring was asked for no list (out_n = 0)"
        return nbest["nbest"]
    if hasattr(nbest, "nbest") and hasattr(nbest, "nlm_logp"):
        assert nbest.nbest is not None, "the rescoring was asked for no list (out_n = 0)"
        return nbest.nbest
    return nbest


def _nbest_arrays(nbest, logp=None, errors=None, need_logp=True):
    """The n-best argument of ctc_mbr_eval, ctc_nbest_consensus and ctc_nbest_rescore: a CtcBeamResult, the dict of ctc_nbest_rescore,
    or a tuple (hyp [S, N, stride], hyp_len [S, N], nbest_count [S], errors [S, N] or None) of int32 CUDA tensors.  logp, errors: the
    caller's own, which go before the result's score and errors (need_logp False: no scores are looked at).  -> hyp, hyp_len, count, errors, logp, S, N, stride, checked."""
    import torch
    nbest = _as_nbest(nbest)
    if isinstance(nbest, CtcBeamResult):
        hyp, hyp_len, count, own_errors, score = nbest.hyp, nbest.hyp_len, nbest.nbest_count, nbest.errors, nbest.score
    else:
        (hyp, hyp_len, count, own_errors), score = nbest, None
    if logp is None:
        logp = score if need_logp else None
    assert logp is not None or not need_logp, "a tuple of lists carries no scores: pass logp"
    if errors is None:
        errors = own_errors
    for t in (hyp, hyp_len, count) + ((errors,) if errors is not None else ()):
        assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()
    assert hyp.dim() == 3 and count.numel() == hyp.shape[0]
    S, N, stride = (int(v) for v in hyp.shape)
    assert hyp_len.shape == (S, N) and (errors is None or errors.shape == (S, N))
    assert logp is None or (logp.is_cuda and logp.dtype == torch.float32 and logp.shape == (S, N) and logp.is_contiguous())
    return hyp, hyp_len, count, errors, logp, S, N, stride


def nbest_to_lists(result):
    """CtcBeamResult (or the dict of ctc_nbest_rescore) -> per stream a list of (hypothesis list, score, errors or None), best first.
    The one place that synchronises."""
    result = _as_nbest(result)
    h, n, c, sc = result.hyp.cpu().numpy(), result.hyp_len.cpu().numpy(), result.nbest_count.cpu().numpy(), result.score.cpu().numpy()
    er = result.errors.cpu().numpy() if result.errors is not None else None
    return [[(h[s, q, :n[s, q]].tolist(), float(sc[s, q]), int(er[s, q]) if er is not None else None) for q in range(c[s])]
            for s in range(len(c))]


CtcStreamResult = collections.namedtuple("CtcStreamResult", "hyp hyp_len nbest_count score errors frames stable_len")


def ctc_beam_stream_state_bytes(max_frames, S, beam):
    return _workspace_bytes("klstm_ctc_beam_stream_state_bytes", max_frames, S, beam)


def ctc_beam_stream_workspace_bytes(T, S, cands, nbest):
    return _workspace_bytes("klstm_ctc_beam_stream_workspace_bytes", T, S, cands, nbest)


class CtcBeamStream:
    """CTC prefix beam search over S streams that is fed chunk by chunk: the beam and the prefix tree of every stream stay on the
    device between the calls (klstm_ctc_beam_stream_step / _emit of include/klstm.h).  K classes, utterances of at most max_frames
    frames; blank, beam, cands, class_weight and lm as ctc_beam_decode takes them.  For any split of an utterance into chunks, emit
    returns the bits ctc_beam_decode returns for the frames consumed so far."""

    def __init__(self, S, K, max_frames, blank=0, beam=16, cands=8, class_weight=None, lm=None, device="cuda"):
        import torch
        self.S, self.K, self.max_frames = int(S), int(K), int(max_frames)
        self.blank, self.beam, self.cands = int(blank), int(beam), int(cands)
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        _check_class_weight(class_weight, self.K)
        assert lm is None or (lm.classes == self.K and _lm_device(lm) == self.device), \
            "the language model's tables have K columns and live on the stream's device"
        self.class_weight, self.lm = class_weight, lm
        self.state_bytes = ctc_beam_stream_state_bytes(self.max_frames, self.S, self.beam)
        self.state = torch.zeros(self.state_bytes, dtype=torch.uint8, device=self.device)          # zero-filled: nothing yet
        self._ws, self._emit_ws = {}, None

    def _workspace(self, T, nbest):
        """one workspace per chunk length"""
        import torch
        nbytes = ctc_beam_stream_workspace_bytes(T, self.S, self.cands, nbest)
        ws = self._ws.get(T)
        if ws is None:
            if len(self._ws) >= 8:
                self._ws.clear()
            ws = self._ws[T] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return ws, nbytes

    def _ints(self, v, what):
        import torch
        if isinstance(v, torch.Tensor) and v.is_cuda:
            assert v.dtype == torch.int32 and v.is_contiguous() and v.numel() == self.S, what
            return v
        v = [int(x) for x in v]
        assert len(v) == self.S, what
        return torch.tensor(v, dtype=torch.int32, device=self.device)

    def step(self, net_out, lens, start=None, stream=None):
        """net_out [T*S, K] float32 CUDA posteriors of one chunk (row t*S + s; a column window with a larger row stride is fine);
        lens: the S frame counts of THIS chunk (0: the stream is idle in this call and its state is not touched); start: None, or S
        flags, nonzero where a new utterance begins with this chunk.  A stream whose utterance would exceed max_frames is rejected
        for the call (emit reports frames = -1 - frames).  Nothing synchronises."""
        import torch
        assert net_out.is_cuda and net_out.dtype == torch.float32 and net_out.dim() == 2 and net_out.stride(1) == 1
        assert net_out.device == self.device and net_out.shape[1] == self.K, "net_out has K columns and lives on the stream's device"
        assert net_out.shape[0] > 0 and net_out.shape[0] % self.S == 0, "rows must be T * S"
        T = net_out.shape[0] // self.S
        lens_dev = self._ints(lens, "lens: S chunk lengths")
        start_dev = self._ints(start, "start: S flags") if start is not None else None
        ws, nbytes = self._workspace(T, 1)
        lm = self.lm
        if isinstance(lm, CtcSparseLabelLm):
            _chk(load_library().klstm_ctc_beam_stream_step_slm(
                net_out.data_ptr(), T, self.S, self.K, net_out.stride(0), lens_dev.data_ptr(), _ptr(start_dev), self.blank,
                _ptr(self.class_weight), self.beam, self.cands, lm.blob.data_ptr(), ctypes.c_size_t(lm.nbytes), lm.states,
                self.state.data_ptr(), ctypes.c_size_t(self.state_bytes), self.max_frames, ws.data_ptr(), ctypes.c_size_t(nbytes), _sp(stream)))
            return
        _chk(load_library().klstm_ctc_beam_stream_step(
            net_out.data_ptr(), T, self.S, self.K, net_out.stride(0), lens_dev.data_ptr(), _ptr(start_dev), self.blank,
            _ptr(self.class_weight), self.beam, self.cands, lm.states if lm else 0, _ptr(lm.next) if lm else None,
            _ptr(lm.weight) if lm else None, self.state.data_ptr(), ctypes.c_size_t(self.state_bytes), self.max_frames, ws.data_ptr(),
            ctypes.c_size_t(nbytes), _sp(stream)))

    def _emit_states(self):
        """the state count emit is told: it reads the final weights alone, so a sparse model (whose states times K may pass the dense
        limit) counts as one state"""
        lm = self.lm
        return 0 if lm is None else 1 if isinstance(lm, CtcSparseLabelLm) else lm.states

    def emit(self, mode, nbest=1, refs=None, totals=None, stream=None):
        """The current n-best lists.  mode: S values, 0 skip the stream (nbest_count 0), 1 the list without the LM's final weights, 2
        with them.  refs, totals as ctc_beam_decode takes them; they cover the streams emitted with mode 2.  Returns
        CtcStreamResult: the fields of CtcBeamResult (hyp [S, N, max_frames]), frames [S] int32 (frames consumed; -1 - frames after an
        overflow) and stable_len [S] int32 (the leading tokens of the 1-best that can no longer change).  Changes nothing in the
        state: call it between any two steps.  Nothing synchronises; nbest_to_lists() does."""
        import torch
        dev, S, nbest = self.device, self.S, int(nbest)
        mode_dev = self._ints(mode, "mode: S values")
        lab_dev = off_dev = errors = None
        if refs is not None:
            lab_dev, off_dev, _ = _packed(refs, S, dev)
        assert totals is None or refs is not None, "totals need refs"
        _check_totals(totals, 6)
        nbytes = ctc_beam_stream_workspace_bytes(1, S, 1, nbest)
        if self._emit_ws is None:
            self._emit_ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)          # its size does not depend on nbest
        ws = self._emit_ws
        hyp = torch.empty(S, max(nbest, 0), self.max_frames, dtype=torch.int32, device=dev)
        hyp_len = torch.empty(S, max(nbest, 0), dtype=torch.int32, device=dev)
        count = torch.empty(S, dtype=torch.int32, device=dev)
        score = torch.empty(S, max(nbest, 0), device=dev)
        frames = torch.empty(S, dtype=torch.int32, device=dev)
        stable = torch.zeros(S, dtype=torch.int32, device=dev)
        if refs is not None:
            errors = torch.empty(S, max(nbest, 0), dtype=torch.int32, device=dev)
        lm = self.lm
        _chk(load_library().klstm_ctc_beam_stream_emit(
            S, self.K, self.blank, self.beam, nbest, mode_dev.data_ptr(), self._emit_states(), _ptr(lm.final) if lm else None,
            self.state.data_ptr(), ctypes.c_size_t(self.state_bytes), self.max_frames, hyp.data_ptr(), self.max_frames, hyp_len.data_ptr(),
            count.data_ptr(), score.data_ptr(), frames.data_ptr(), stable.data_ptr(), _ptr(lab_dev), _ptr(off_dev), _ptr(errors),
            _ptr(totals), ws.data_ptr(), ctypes.c_size_t(nbytes), _sp(stream)))
        return CtcStreamResult(hyp, hyp_len, count, score, errors, frames, stable)


CtcMbrResult = collections.namedtuple("CtcMbrResult", "risk diff hyp_logp hyp_post ref_loss")


def ctc_mbr_workspace_bytes(T, S, list_n, max_len, with_ref=False):
    return _workspace_bytes("klstm_ctc_mbr_workspace_bytes", T, S, list_n, max_len, 1 if with_ref else 0)


def ctc_mbr_eval(net_out, lens, nbest, refs=None, blank=0, risk_scale=1.0, ctc_weight=0.0, max_len=None, diff=None, totals=None, stream=None):
    """Minimum expected token error over n-best lists: net_out, lens as ctc_eval takes them; nbest: the CtcBeamResult of ctc_beam_decode
    on the same posteriors (decoded with refs, so that it carries the edit distances), or a tuple (hyp [S, N, stride] int32, hyp_len
    [S, N], nbest_count [S], errors [S, N]) of int32 CUDA tensors; refs: the reference labels (a list, or what pack_labels() returned),
    needed exactly when ctc_weight > 0.  With P = softmax over the list of risk_scale * log p(h_q | y) and R = sum_q P_q errors_q:
    diff = the gradient of R + ctc_weight * (-log p(ref | y)) with respect to the softmax input.  max_len: the label capacity the
    workspace is sized for (an entry longer than the capacity that follows from the workspace's size, max_len or a label or two more, is
    dropped; the workspace grows with it: pass it.  None: min(1023, 2 * longest reference + 8)
    with refs, else min(1023, the hypothesis stride), which no entry exceeds).  Returns
    CtcMbrResult(risk [S] float32 (0 idle, -1 rejected or skipped), diff [T*S, K], hyp_logp [S, N] float32 (-inf: dropped), hyp_post
    [S, N] float32, ref_loss [S] float32 or None).  totals: a float64[6] CUDA tensor that sum of R, sum of the 1-best's errors,
    utterances counted, utterances rejected or skipped, frames and sum of the reference losses are added to.  Nothing synchronises."""
    import torch
    lib = load_library()
    dev = net_out.device
    lens_dev, S, T, K = _shape(net_out, lens)
    hyp, hyp_len, count, errors, _, Sn, N, hyp_stride = _nbest_arrays(nbest, need_logp=False)
    assert errors is not None, "the n-best lists carry no edit distances (decode with refs)"
    assert Sn == S
    with_ref = float(ctc_weight) > 0
    lab_dev = off_dev = ref_loss = None
    longest = 0
    if with_ref:
        assert refs is not None, "ctc_weight > 0 needs refs"
        lab_dev, off_dev, longest = _packed(refs, S, dev)
        ref_loss = torch.empty(S, device=dev)
    if max_len is None:
        max_len = min(1023, 2 * longest + 8 if with_ref else hyp_stride)
    if diff is None:
        diff = torch.empty(T * S, K, device=dev)
    assert diff.is_cuda and diff.dtype == torch.float32 and diff.shape == (T * S, K) and diff.stride(1) == 1
    _check_totals(totals, 6)
    nbytes = ctc_mbr_workspace_bytes(T, S, N, max_len, with_ref)
    ws = _workspace("mbr", (T, S, N, max_len, with_ref), nbytes, dev)
    risk = torch.empty(S, device=dev)
    hyp_logp = torch.empty(S, N, device=dev)
    hyp_post = torch.empty(S, N, device=dev)
    _chk(lib.klstm_ctc_mbr_eval(net_out.data_ptr(), T, S, K, net_out.stride(0), lens_dev.data_ptr(), int(blank), hyp.data_ptr(), hyp_stride,
                                hyp_len.data_ptr(), count.data_ptr(), errors.data_ptr(), N, _ptr(lab_dev), _ptr(off_dev), float(risk_scale),
                                float(ctc_weight), diff.data_ptr(), diff.stride(0), risk.data_ptr(), hyp_logp.data_ptr(), hyp_post.data_ptr(),
                                _ptr(ref_loss), _ptr(totals), ws.data_ptr(), ctypes.c_size_t(nbytes), _sp(stream)))
    return CtcMbrResult(risk, diff, hyp_logp, hyp_post, ref_loss)


CtcConsensusResult = collections.namedtuple("CtcConsensusResult", "pick map mbr post risk unit_len conf dist")


def ctc_consensus_workspace_bytes(S, list_n, max_len, word_mode=False):
    return _workspace_bytes("klstm_ctc_consensus_workspace_bytes", S, list_n, max_len, 1 if word_mode else 0)


def ctc_nbest_consensus(nbest, logp=None, scale=1.0, separator=None, pivot="mbr", errors=None, max_len=None, want_dist=False, totals=None,
                        stream=None):
    """Minimum Bayes risk decoding and unit confidences over n-best lists (klstm_ctc_consensus of include/klstm.h, which defines every
    quantity).  nbest: the CtcBeamResult of ctc_beam_decode, or a tuple (hyp [S, N, stride] int32, hyp_len [S, N], nbest_count [S],
    errors [S, N] or None) of CUDA tensors as ctc_mbr_eval takes it; logp [S, N] float32: the natural-log weights of the entries (None:
    the result's score; ctc_mbr_eval(...).hyp_logp are the exact ones); scale multiplies them; separator: None for token units, or
    the class that separates words (the lists of a lexicon_label_lm search); pivot: "map" or "mbr"; errors: None (the result's, if it
    has them) or [S, N] int32; max_len: the token capacity (None: min(1023, stride)).  Returns CtcConsensusResult(pick, map, mbr [S]
    int32 (-1: idle or rejected), post [S, N] float32, risk [S, N] float32 (-1: dropped), unit_len [S, N] int32, conf [S, stride]
    float32 (valid up to unit_len[s, pick[s]]), dist [S, N, N] int32 or None without want_dist).  totals: a float64[10] CUDA tensor that
    streams done, streams idle or rejected, sum of R[pick], sum of R[map], streams with mbr != map, the picks' units, sum of conf over
    them, entries dropped, sum of errors[pick] and sum of errors[map] are added to.  Nothing synchronises; consensus_to_lists() does."""
    import torch
    lib = load_library()
    hyp, hyp_len, count, errors, logp, S, N, stride = _nbest_arrays(nbest, logp, errors)
    dev = hyp.device
    assert pivot in ("map", "mbr")
    sep = -1 if separator is None else int(separator)
    assert separator is None or sep >= 0, "the separator is a class"
    if max_len is None:
        max_len = min(1023, stride)
    max_len = int(max_len)
    _check_totals(totals, 10)
    nbytes = ctc_consensus_workspace_bytes(S, N, max_len, sep >= 0)
    ws = _workspace("consensus", (S, N, max_len, sep >= 0), nbytes, dev)
    pick, imap, imbr = (torch.empty(S, dtype=torch.int32, device=dev) for _ in range(3))
    post, risk = torch.empty(S, N, device=dev), torch.empty(S, N, device=dev)
    unit_len = torch.empty(S, N, dtype=torch.int32, device=dev)
    conf = torch.zeros(S, max(stride, 1), device=dev)
    dist = torch.empty(S, N, N, dtype=torch.int32, device=dev) if want_dist else None
    _chk(lib.klstm_ctc_consensus(hyp.data_ptr(), max(stride, 1), hyp_len.data_ptr(), count.data_ptr(), logp.data_ptr(), _ptr(errors), S, N, max_len,
                                 float(scale), sep, 1 if pivot == "mbr" else 0, pick.data_ptr(), imap.data_ptr(), imbr.data_ptr(),
                                 post.data_ptr(), risk.data_ptr(), unit_len.data_ptr(), conf.data_ptr(), conf.stride(0), _ptr(dist),
                                 _ptr(totals), ws.data_ptr(), ctypes.c_size_t(nbytes), _sp(stream)))
    return CtcConsensusResult(pick, imap, imbr, post, risk, unit_len, conf, dist)


def consensus_to_lists(result, nbest, separator=None):
    """CtcConsensusResult and the lists it was computed from -> per stream None (idle or rejected), or a dict(pick, units: a list of
    (unit, confidence) with unit a token (separator None) or the list of a word's tokens, risk: the pick's expected unit errors).  The
    one place that synchronises."""
    hyp, hyp_len = (nbest.hyp, nbest.hyp_len) if isinstance(nbest, CtcBeamResult) else nbest[:2]
    h, n = hyp.cpu().numpy(), hyp_len.cpu().numpy()
    pick, risk, conf = result.pick.cpu().numpy(), result.risk.cpu().numpy(), result.conf.cpu().numpy()
    out = []
    for s, p in enumerate(pick):
        if p < 0:
            out.append(None)
            continue
        toks = h[s, p, :n[s, p]].tolist()
        units = toks if separator is None else split_words(toks, int(separator))
        out.append(dict(pick=int(p), units=[(u, float(conf[s, i])) for i, u in enumerate(units)], risk=float(risk[s, p])))
    return out


class CtcWordTable:
    """The device arrays of a word table for ctc_nbest_rescore(words=...): keys uint64 [W] ascending and ids int32 [W] as
    lm.word_table() returns them, the class unk_id an unknown word takes (negative: it forbids the entry) and the separator class."""

    def __init__(self, keys, ids, unk_id, separator, device="cuda"):
        import torch
        keys, ids = np.ascontiguousarray(keys, np.uint64), np.ascontiguousarray(ids, np.int32)
        assert keys.ndim == 1 and keys.shape == ids.shape and keys.size >= 1
        self.keys = torch.from_numpy(keys.view(np.int64)).to(device)               # the bits; the device reads them unsigned
        self.ids = torch.from_numpy(ids).to(device)
        self.words, self.unk_id, self.separator = int(keys.size), int(unk_id), int(separator)
        assert self.separator >= 0, "the separator is a class"


def ctc_rescore_workspace_bytes(S, list_n, max_len, word_mode=False):
    return _workspace_bytes("klstm_ctc_rescore_workspace_bytes", S, list_n, max_len, 1 if word_mode else 0)


def ctc_nbest_rescore(nbest, add=None, sub=None, words=None, am_scale=1.0, add_scale=1.0, unit_bonus=0.0, out_n=None, max_len=None,
                      totals=None, stream=None, logp=None, out_stride=None, classes=None):
    """Second-pass rescoring of n-best lists (klstm_ctc_nbest_rescore of include/klstm.h, which defines every quantity).  nbest: the
    CtcBeamResult of ctc_beam_decode, or a tuple (hyp [S, N, stride] int32, hyp_len [S, N], nbest_count [S], errors [S, N] or None) of
    CUDA tensors with logp [S, N] float32 given, or the dict of an earlier rescoring (its re-ranked list).  sub: None, or the CtcSparseLabelLm the first pass fused, whose score is taken out;
    add: None, or the CtcSparseLabelLm whose score is put in -- over the tokens, or with words (a CtcWordTable) over the words, its
    reserved class being the blank it was built with.  z = am_scale * logp - logw(sub) + add_scale * logw(add) + unit_bonus * units.
    out_n: how many entries of the ranking the re-ranked list keeps (None: N; 0: none); classes: the token classes K (None: sub's, or
    a token-level add's).  Returns a dict: order [S, N] int32 (the entry of rank r, -1 beyond live_count), live_count [S], score [S, N]
    float32 (-inf: dropped, forbidden or unlisted), add_logp, sub_logp [S, N] float32, units, oov [S, N] int32, and nbest: the
    re-ranked list as a CtcBeamResult (None with out_n = 0); ctc_nbest_consensus, ctc_mbr_eval and nbest_to_lists take the dict in
    place of the search's result.  totals: a float64[8] CUDA tensor that streams done, streams idle or rejected, entries dropped,
    entries forbidden, streams whose 1-best changed, the errors of the first pass's 1-best, the errors of the new 1-best and words out
    of vocabulary are added to.  Nothing synchronises."""
    import torch
    lib = load_library()
    hyp, hyp_len, count, errors, logp, S, N, stride = _nbest_arrays(nbest, logp)
    dev = hyp.device
    for m in (add, sub):
        assert m is None or (isinstance(m, CtcSparseLabelLm) and m.blob.device == dev), "the models are CtcSparseLabelLm on the lists' device"
    assert words is None or isinstance(words, CtcWordTable)
    if classes is None:
        classes = sub.classes if sub is not None else add.classes if (add is not None and words is None) else None
    assert classes is not None, "word-level rescoring without sub: pass classes, the number of token classes"
    if max_len is None:
        max_len = min(1023, stride)
    max_len = int(max_len)
    out_n = N if out_n is None else int(out_n)
    _check_totals(totals, 8)
    nbytes = ctc_rescore_workspace_bytes(S, N, max_len, words is not None)
    ws = _workspace("rescore", (S, N, max_len), nbytes, dev)
    order = torch.empty(S, N, dtype=torch.int32, device=dev)
    live = torch.empty(S, dtype=torch.int32, device=dev)
    z, add_logp, sub_logp = (torch.empty(S, N, device=dev) for _ in range(3))
    units, oov = (torch.empty(S, N, dtype=torch.int32, device=dev) for _ in range(2))
    out = None
    if out_n >= 1:
        out_stride = max(min(stride, max_len), 1) if out_stride is None else int(out_stride)
        n1 = max(out_n, 1)
        out = CtcBeamResult(torch.zeros(S, n1, out_stride, dtype=torch.int32, device=dev), torch.zeros(S, n1, dtype=torch.int32, device=dev),
                            torch.zeros(S, dtype=torch.int32, device=dev), torch.full((S, n1), -np.inf, device=dev),
                            torch.full((S, n1), -1, dtype=torch.int32, device=dev) if errors is not None else None)
    _chk(lib.klstm_ctc_nbest_rescore(
        hyp.data_ptr(), max(stride, 1), hyp_len.data_ptr(), count.data_ptr(), logp.data_ptr(), _ptr(errors), S, N, max_len, int(classes),
        sub.blob.data_ptr() if sub else None, ctypes.c_size_t(sub.nbytes if sub else 0), sub.states if sub else 0, _ptr(sub.final) if sub else None,
        add.blob.data_ptr() if add else None, ctypes.c_size_t(add.nbytes if add else 0), add.states if add else 0, add.classes if add else 0,
        _ptr(add.final) if add else None, words.keys.data_ptr() if words else None, words.ids.data_ptr() if words else None,
        words.words if words else 0, words.unk_id if words else -1, words.separator if words else -1, add.blank if (add and words) else -1,
        float(am_scale), float(add_scale), float(unit_bonus), order.data_ptr(), live.data_ptr(), z.data_ptr(), add_logp.data_ptr(),
        sub_logp.data_ptr(), units.data_ptr(), oov.data_ptr(), out_n, _ptr(out.hyp) if out else None, out_stride if out else 0,
        _ptr(out.hyp_len) if out else None, _ptr(out.nbest_count) if out else None, _ptr(out.score) if out else None,
        _ptr(out.errors) if out else None, _ptr(totals), ws.data_ptr(), ctypes.c_size_t(nbytes), _sp(stream)))
    return dict(order=order, live_count=live, score=z, add_logp=add_logp, sub_logp=sub_logp, units=units, oov=oov, nbest=out)


CtcMmiResult = collections.namedtuple("CtcMmiResult", "loss diff num_logp den_logz lm_logw")


def ctc_mmi_workspace_bytes(T, S, K, lm_states, max_label_len):
    return _workspace_bytes("klstm_ctc_mmi_workspace_bytes", T, S, K, lm_states, max_label_len)


class CtcMmiDenominator:
    """The denominator graph of ctc_mmi_eval for one language model: built on the device from the tables of a CtcLabelLm (the object
    ctc_beam_decode(lm=...) takes) and kept for every minibatch of a training run (klstm_ctc_mmi_graph_build of include/klstm.h).
    Owns the graph's buffer; the tables are not needed afterwards.  The dense model only: a CtcSparseLabelLm is for the search, and a
    small one reaches MMI through CtcLabelLm(*lm.sparse_lm_to_dense(model))."""

    def __init__(self, lm, blank=0, stream=None):
        import torch
        self.states, self.classes, self.blank = lm.states, lm.classes, int(blank)
        self.device = lm.next.device
        n = getattr(load_library(), "klstm_ctc_mmi_graph_bytes")(self.states, self.classes)
        if n == 0:
            _chk(2)
        self.graph_bytes = n
        self.graph = torch.empty(n, dtype=torch.uint8, device=self.device)
        _chk(load_library().klstm_ctc_mmi_graph_build(self.states, self.classes, self.blank, lm.next.data_ptr(), lm.weight.data_ptr(),
                                                     _ptr(lm.final), self.graph.data_ptr(), ctypes.c_size_t(n), _sp(stream)))


def ctc_mmi_eval(net_out, lens, labels, den, ctc_weight=0.0, diff=None, totals=None, stream=None):
    """MMI (CTC-CRF) against the language model of `den` (a CtcMmiDenominator): net_out, lens, labels as ctc_eval takes them.  loss =
    -log p_ctc(labels | y) - log W(labels) + log Z with Z summed over every labelling the model accepts; diff = gamma_den - gamma_ref +
    ctc_weight * (y - gamma_ref), the gradient with respect to the softmax input.  Returns CtcMmiResult(loss [S] float32 (0 idle, +inf
    rejected: what ctc_eval rejects, and labels the model does not accept), diff [T*S, K], num_logp [S] (the bits of -utt_loss of
    ctc_eval), den_logz [S], lm_logw [S]; the last three 0 on streams that are not counted).  totals: a float64[5] CUDA tensor that sum
    of loss, utterances counted, utterances rejected, frames and sum of -num_logp are added to.  Nothing synchronises."""
    import torch
    lib = load_library()
    dev = net_out.device
    lens_dev, S, T, K = _shape(net_out, lens)
    assert den.classes == K and den.device == dev, "the denominator was built for K classes on net_out's device"
    lab_dev, off_dev, longest = _packed(labels, S, dev)
    if diff is None:
        diff = torch.empty(T * S, K, device=dev)
    assert diff.is_cuda and diff.dtype == torch.float32 and diff.shape == (T * S, K) and diff.stride(1) == 1
    _check_totals(totals, 5)
    cap = min(longest, 1023)                                            # a longer sequence is the device's to reject
    nbytes = ctc_mmi_workspace_bytes(T, S, K, den.states, cap)
    ws = _workspace("mmi", (T, S, K, den.states, cap), nbytes, dev)
    loss, num_logp, den_logz, lm_logw = (torch.empty(S, device=dev) for _ in range(4))
    _chk(lib.klstm_ctc_mmi_eval(net_out.data_ptr(), T, S, K, net_out.stride(0), lens_dev.data_ptr(), lab_dev.data_ptr(), off_dev.data_ptr(),
                                den.blank, den.graph.data_ptr(), ctypes.c_size_t(den.graph_bytes), den.states, float(ctc_weight),
                                diff.data_ptr(), diff.stride(0), loss.data_ptr(), num_logp.data_ptr(), den_logz.data_ptr(),
                                lm_logw.data_ptr(), _ptr(totals), ws.data_ptr(), ctypes.c_size_t(nbytes), _sp(stream)))
    return CtcMmiResult(loss, diff, num_logp, den_logz, lm_logw)
