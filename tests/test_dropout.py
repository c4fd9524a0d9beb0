"""Forward-connection dropout without a GPU (include/klstm_dropout.h, the <Dropout> component of include/klstm_nnet.hpp): the numpy
twin against the published known answers of Philox4x32-10, the threshold rule of kdrop_threshold against the twin, every argument
refusal of kdrop_apply, the exported names, model files with <Dropout> in them, and the statistics of the mask."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import cpp_driver, dropout_fmt, dropout_ref, kaldi_fmt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ("klstm.h", "klstm_dropout.h", "klstm_component.hpp", "klstm_kaldi_io.hpp", "klstm_trainer.hpp", "klstm_nnet.hpp", "klstm_scorer.hpp")


@pytest.fixture(autouse=True, scope="module")
def the_library_has_the_family():
    """the twin is the executable form of a contract the library must carry: nothing here passes against a library without it"""
    import kaldi_lstm_amd as k
    lib = k.load_library()
    assert hasattr(lib, "kdrop_threshold") and hasattr(lib, "kdrop_apply"), "libklstm.so has no kdrop_* entries"
    assert os.path.exists(os.path.join(ROOT, "include", "klstm_dropout.h"))


def build_dropout_driver():
    return cpp_driver.build("dropout_test", headers=HEADERS)


def run(*args, ok=True):
    return cpp_driver.run("dropout_test", *args, ok=ok, headers=HEADERS)


def test_twin_reproduces_the_known_answers_of_philox4x32_10():
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        assert " ".join("%08x" % int(w) for w in dropout_ref.philox4x32_10(*ctr, *key)) == want
    # vectorised over counters: the same words as one call per counter
    w = dropout_ref.philox4x32_10(np.array([0, 0x243f6a88]), np.array([0, 0x85a308d3]), np.array([0, 0x13198a2e]), np.array([0, 0x03707344]), 0, 0)
    assert "%08x" % int(w[0][0]) == "6627e8d5"


def test_threshold_rule_is_the_twins():
    import kaldi_lstm_amd as k
    f32 = np.float32
    for p in (f32(0.8), f32(0.5), f32(1) / f32(3), np.nextafter(f32(1), f32(0)), f32(2.0 ** -32), f32(1)):
        thr, scale = k.dropout_threshold(p)
        want_thr, want_scale = dropout_ref.threshold(p)
        assert thr == want_thr and f32(scale).view(np.uint32) == want_scale.view(np.uint32), p
    assert k.dropout_threshold(f32(0.5)) == (2 ** 31, 2.0) and k.dropout_threshold(1.0) == (2 ** 32 - 1, 1.0)
    assert k.dropout_threshold(2.0 ** -32) == (1, 2.0 ** 32)
    for p in (0.0, -0.1, f32(1.0000001), float("nan")):
        assert dropout_ref.threshold(p) is None
        with pytest.raises(k.KlstmError) as ei:
            k.dropout_threshold(p)
        assert ei.value.status == 1 and "kdrop_threshold: retention" in str(ei.value)


def test_every_refusal_of_kdrop_apply_answers_before_any_hip_call():
    """tests/cpp/dropout_test.cpp errors: every KLSTM_ERR_ARG case with host pointers that are never followed and no device in the
    machine; messages: each case leaves a message of its own in klstm_last_error()"""
    assert run("errors").stdout.startswith("OK 23 refusals")
    lines = run("messages").stdout.splitlines()[1:]
    assert len(lines) == 10
    msgs = [ln.split("|", 1) for ln in lines]
    assert all(st == "1" and m.startswith("kdrop_apply: ") for st, m in msgs)
    assert len({m for _, m in msgs}) == len(msgs)


def test_exported_kdrop_names_are_the_recorded_list():
    import kaldi_lstm_amd as k
    out = subprocess.run(["nm", "-D", "--defined-only", k.lib_path()], capture_output=True, text=True, check=True).stdout
    have = sorted({ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("kdrop_")})
    want = open(os.path.join(ROOT, "tests", "golden", "kdrop_abi_names.txt")).read().split()
    assert want == ["kdrop_apply", "kdrop_threshold"] and have == want
    lib = k.load_library()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "klstm_dropout.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(kdrop_[a-z_0-9]+)\s*\(", hdr))) == want and all(hasattr(lib, n) for n in want)
    assert "kdrop_" not in open(os.path.join(ROOT, "include", "klstm.h")).read()        # a family of its own, like knlm_*


# ---- model files (host only) ----
I, C, R, NPDF, S = 8, 4, 8, 5, 3


def dyadic(shape, seed):
    """multiples of 1/8 in [-1, 1]: the same digits in %.9g and in a stream's six"""
    return (np.random.RandomState(seed).randint(-8, 9, size=shape) / 8.0).astype(np.float32)


def make_layers():
    nparams = 4 * C * I + 4 * C * R + 4 * C + 3 * C + R * C
    return [("transmit", I), ("lstm_streams", dyadic(nparams, 1), I, C, R, S), ("dropout", R, 0.8), ("lstm_streams", dyadic(nparams, 2), R, C, R, S),
            ("dropout", R, 0.5), ("affine", dyadic((NPDF, R), 3), dyadic(NPDF, 4)), ("softmax", NPDF)]


def test_model_with_dropout_roundtrips_text_binary_text(tmp_path):
    layers = make_layers()
    text, binary = dropout_fmt.nnet_text(layers), dropout_fmt.nnet_binary(layers)
    assert b"\n<Dropout> 8 8 <DropoutRetention> 0.8 \n" in text                      # the text form, by hand
    assert b"<Dropout> \x04\x08\x00\x00\x00\x04\x08\x00\x00\x00<DropoutRetention> \x04\xcd\xcc\x4c\x3f" in binary   # 0.8f = 0x3f4ccccd
    (tmp_path / "n.txt").write_bytes(text)
    out = run("nnet_copy", tmp_path / "n.txt", 1, tmp_path / "n.bin").stdout.split()
    assert out == ["OK", "7", "2", "<Transmit>", "<LstmProjectedStreams>", "<Dropout>", "<LstmProjectedStreams>", "<Dropout>", "<AffineTransform>", "<Softmax>"]
    assert (tmp_path / "n.bin").read_bytes() == binary
    run("nnet_copy", tmp_path / "n.bin", 0, tmp_path / "n2.txt")
    assert (tmp_path / "n2.txt").read_bytes() == text
    run("nnet_copy", tmp_path / "n2.txt", 1, tmp_path / "n2.bin")
    assert (tmp_path / "n2.bin").read_bytes() == binary


@pytest.mark.parametrize("body,why", [("<Dropout> 8 8 \n", "<DropoutRetention>"), ("<Dropout> 8 8 <Retention> 0.8 \n", "<DropoutRetention>"),
                                      ("<Dropout> 8 8 <DropoutRetention> 0 \n", "outside (0, 1]"), ("<Dropout> 8 8 <DropoutRetention> 1.5 \n", "outside (0, 1]"),
                                      ("<Dropout> 8 8 <DropoutRetention> nan \n", "unreadable scalar"), ("<Dropout> 8 4 <DropoutRetention> 0.5 \n", "input dim")])
def test_a_bad_dropout_component_is_refused(tmp_path, body, why):
    (tmp_path / "n.txt").write_bytes(b"<Nnet> \n<Transmit> 8 8 \n" + body.encode() + b"<Softmax> 8 8 \n</Nnet> \n")
    r = run("nnet_copy", tmp_path / "n.txt", 1, tmp_path / "n.bin", ok=False)
    assert r.returncode == 3 and r.stdout.startswith("EXCEPTION:") and why in r.stdout, r.stdout


def test_without_dropout_and_convert_to_standard_give_the_model_without_them(tmp_path):
    layers = make_layers()
    plain = dropout_fmt.without_dropout(layers)
    (tmp_path / "n.bin").write_bytes(dropout_fmt.nnet_binary(layers))
    assert run("without", tmp_path / "n.bin", tmp_path / "w.bin").stdout.split() == ["OK", "5", "0"]
    assert (tmp_path / "w.bin").read_bytes() == kaldi_fmt.nnet_binary(plain)
    assert run("standard", tmp_path / "n.bin", 2, tmp_path / "s.bin").stdout.split() == ["OK", "5", "0"]
    std = [("timeshift", I, 2)] + [("lstm",) + l[1:5] if l[0] == "lstm_streams" else l for l in plain[1:]]
    assert (tmp_path / "s.bin").read_bytes() == kaldi_fmt.nnet_binary(std)


def test_scorer_and_rescorer_refusals_name_without_dropout(tmp_path):
    (tmp_path / "n.bin").write_bytes(dropout_fmt.nnet_binary(make_layers()))
    (tmp_path / "lm.bin").write_bytes(dropout_fmt.nnet_binary(make_layers()[1:]))          # a language model has no <Transmit>
    out = dict(ln.split(": ", 1) for ln in run("topology", tmp_path / "n.bin", tmp_path / "lm.bin").stdout.splitlines()[1:])
    assert "BatchScorer: <Dropout> at component 2" in out["scorer"] and "WithoutDropout" in out["scorer"]
    assert "CtcNeuralRescorer: <Dropout> at component" in out["rescorer"] and "WithoutDropout" in out["rescorer"]
    assert out["scorer_plain"] == ""                       # no refusal: the WithoutDropout form is accepted


def test_set_dropout_retention_reaches_every_dropout_and_leaves_them_off(tmp_path):
    (tmp_path / "n.bin").write_bytes(dropout_fmt.nnet_binary(make_layers()))
    assert run("retention", tmp_path / "n.bin", 0.25, tmp_path / "r.txt").stdout.split() == ["OK", "2", "off"]
    assert (tmp_path / "r.txt").read_bytes().count(b"<Dropout> 8 8 <DropoutRetention> 0.25 \n") == 2
    r = run("retention", tmp_path / "n.bin", 0, tmp_path / "r.txt", ok=False)
    assert r.returncode == 3 and "outside (0, 1]" in r.stdout


# ---- statistics of the mask, on the twin ----
ROWS, COLS, SEED, STEP, SALT = 64, 512, 1234, 3, 1


def sigmas(share, p, n):
    return abs(share - p) / np.sqrt(p * (1 - p) / n)


@pytest.mark.parametrize("p", [0.5, 0.8, 0.95])
def test_kept_share_is_the_retention(p):
    m = dropout_ref.mask(ROWS, COLS, np.float32(p), SEED, STEP, SALT)
    s = sigmas(m.mean(), float(np.float32(p)), m.size)
    print("p", p, "kept share", m.mean(), "sigmas", s)
    assert s <= 4.0


def test_masks_of_other_counters_are_independent():
    p = np.float32(0.5)
    m = dropout_ref.mask(ROWS, COLS, p, SEED, STEP, SALT)
    others = dict(step=dropout_ref.mask(ROWS, COLS, p, SEED, STEP + 1, SALT), salt=dropout_ref.mask(ROWS, COLS, p, SEED, STEP, SALT + 1),
                  seed=dropout_ref.mask(ROWS, COLS, p, SEED + 1, STEP, SALT), seed_high=dropout_ref.mask(ROWS, COLS, p, SEED + 2 ** 32, STEP, SALT))
    pairs = {k: (m, o) for k, o in others.items()}
    pairs["rows"] = (m[:-1], m[1:])
    pairs["cols"] = (m[:, :-1], m[:, 1:])
    for k, (a, b) in pairs.items():
        s = sigmas((a == b).mean(), 0.5, a.size)
        print(k, "agreement", (a == b).mean(), "sigmas", s)
        assert s <= 4.0, k


def test_sequence_mode_of_the_twin_holds_one_mask_per_stream_and_id():
    p, T, S_ = np.float32(0.5), 5, 3
    m = dropout_ref.mask(T * S_, 37, p, SEED, 9, SALT, dropout_ref.SEQUENCE, S_, [7, 7, 9]).reshape(T, S_, 37)
    assert (m == m[0]).all() and (m[0, 0] == m[0, 1]).all() and not (m[0, 0] == m[0, 2]).all()
    assert (m == dropout_ref.mask(T * S_, 37, p, SEED, 0, SALT, dropout_ref.SEQUENCE, S_, [7, 7, 9]).reshape(T, S_, 37)).all()   # step plays no part
    assert not (m.reshape(T * S_, 37) == dropout_ref.mask(T * S_, 37, p, SEED, 0, SALT)).all()
