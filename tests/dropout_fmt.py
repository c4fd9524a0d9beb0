"""Kaldi nnet1 model bytes with <Dropout> components in them, assembled independently of include/klstm_nnet.hpp: the layers of
tests/kaldi_fmt.py plus ("dropout", dim, retention).  Binary: token, int32 dims, "<DropoutRetention> ", a float; text:
"<Dropout> 8 8 <DropoutRetention> 0.8 " and a newline."""
import struct

from tests import kaldi_fmt

_HEAD_B, _TAIL_B = b"\x00B<Nnet> ", b"</Nnet> "
_HEAD_T, _TAIL_T = b"<Nnet> \n", b"</Nnet> \n"


def _one_binary(l):
    if l[0] == "dropout":
        return b"<Dropout> " + kaldi_fmt._i32(l[1]) + kaldi_fmt._i32(l[1]) + b"<DropoutRetention> " + b"\x04" + struct.pack("<f", l[2])
    body = kaldi_fmt.nnet_binary([l])
    assert body.startswith(_HEAD_B) and body.endswith(_TAIL_B)
    return body[len(_HEAD_B):-len(_TAIL_B)]


def _one_text(l):
    if l[0] == "dropout":
        return ("<Dropout> %d %d <DropoutRetention> %g \n" % (l[1], l[1], l[2])).encode()
    body = kaldi_fmt.nnet_text([l])
    assert body.startswith(_HEAD_T) and body.endswith(_TAIL_T)
    return body[len(_HEAD_T):-len(_TAIL_T)]


def nnet_binary(layers):
    return _HEAD_B + b"".join(_one_binary(l) for l in layers) + _TAIL_B


def nnet_text(layers):
    return _HEAD_T + b"".join(_one_text(l) for l in layers) + _TAIL_T


def without_dropout(layers):
    return [l for l in layers if l[0] != "dropout"]
