"""Kaldi nnet1 model bytes with the CLDNN front-end components in them, assembled independently of include/klstm_nnet.hpp: the layers
of tests/kaldi_fmt.py plus
  ("conv", filters [F x K], bias [F], in_dim, out_dim, patch_dim, patch_step, patch_stride)
  ("pool", in_dim, out_dim, pool_size, pool_step, pool_stride) | ("sigmoid", dim) | ("tanh", dim)
Text: "<ConvolutionalComponent> 104 48 <PatchDim> 4 <PatchStep> 1 <PatchStride> 16 <LearnRateCoef> 1 <BiasLearnRateCoef> 1 <MaxNorm> 0
<Filters>  [ ... ]" newline "<Bias>  [ ... ]"; "<MaxPoolingComponent> 32 104 <PoolSize> 3 <PoolStep> 3 <PoolStride> 8 "; "<Sigmoid> 32 32 "."""
from tests import kaldi_fmt
from tests.kaldi_fmt import _f32, _i32, _mat, _tmat, _tok, _tvec, _vec

_HEAD_B, _TAIL_B = b"\x00B<Nnet> ", b"</Nnet> "
_HEAD_T, _TAIL_T = b"<Nnet> \n", b"</Nnet> \n"
_PLAIN = {"sigmoid": "<Sigmoid>", "tanh": "<Tanh>"}


def _one_binary(l):
    if l[0] == "conv":
        _, W, b, din, dout, pd, ps, st = l
        return (_tok("<ConvolutionalComponent>") + _i32(dout) + _i32(din) + _tok("<PatchDim>") + _i32(pd) + _tok("<PatchStep>") + _i32(ps) +
                _tok("<PatchStride>") + _i32(st) + _tok("<LearnRateCoef>") + _f32(1.0) + _tok("<BiasLearnRateCoef>") + _f32(1.0) +
                _tok("<MaxNorm>") + _f32(0.0) + _tok("<Filters>") + _mat(W) + _tok("<Bias>") + _vec(b))
    if l[0] == "pool":
        _, din, dout, z, g, w = l
        return _tok("<MaxPoolingComponent>") + _i32(dout) + _i32(din) + _tok("<PoolSize>") + _i32(z) + _tok("<PoolStep>") + _i32(g) + _tok("<PoolStride>") + _i32(w)
    if l[0] in _PLAIN:
        return _tok(_PLAIN[l[0]]) + _i32(l[1]) + _i32(l[1])
    body = kaldi_fmt.nnet_binary([l])
    assert body.startswith(_HEAD_B) and body.endswith(_TAIL_B)
    return body[len(_HEAD_B):-len(_TAIL_B)]


def _one_text(l, order=None):
    if l[0] == "conv":
        _, W, b, din, dout, pd, ps, st = l
        toks = {"<PatchDim>": "%d" % pd, "<PatchStep>": "%d" % ps, "<PatchStride>": "%d" % st, "<LearnRateCoef>": "1", "<BiasLearnRateCoef>": "1", "<MaxNorm>": "0"}
        order = order or ["<PatchDim>", "<PatchStep>", "<PatchStride>", "<LearnRateCoef>", "<BiasLearnRateCoef>", "<MaxNorm>"]
        s = "<ConvolutionalComponent> %d %d " % (dout, din) + "".join("%s %s " % (t, toks[t]) for t in order)
        return (s + "<Filters> " + _tmat(W) + "<Bias> " + _tvec(b)).encode()
    if l[0] == "pool":
        return ("<MaxPoolingComponent> %d %d <PoolSize> %d <PoolStep> %d <PoolStride> %d \n" % (l[2], l[1], l[3], l[4], l[5])).encode()
    if l[0] in _PLAIN:
        return ("%s %d %d \n" % (_PLAIN[l[0]], l[1], l[1])).encode()
    body = kaldi_fmt.nnet_text([l])
    assert body.startswith(_HEAD_T) and body.endswith(_TAIL_T)
    return body[len(_HEAD_T):-len(_TAIL_T)]


def nnet_binary(layers):
    return _HEAD_B + b"".join(_one_binary(l) for l in layers) + _TAIL_B


def nnet_text(layers, conv_token_order=None):
    """conv_token_order: another order of the tokens before <Filters> (a reader must accept any; a writer uses the default)"""
    return _HEAD_T + b"".join(_one_text(l, conv_token_order) for l in layers) + _TAIL_T
