"""Batched scoring, host side (include/klstm_scorer.hpp through tests/cpp/scorer_test; no GPU): FAQ Q1's google -> standard
conversion as code, the scorer's refusal of models and options it does not take, and the chunk plan against a numpy restatement."""
import os
import subprocess

import numpy as np
import pytest

from oracle.oracle import make_params
from tests import kaldi_fmt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "scorer_test")
SRC = EXE + ".cpp"
HDRS = [os.path.join(ROOT, "include", h) for h in ("klstm.h", "klstm_component.hpp", "klstm_kaldi_io.hpp", "klstm_trainer.hpp",
                                                   "klstm_nnet.hpp", "klstm_scorer.hpp")]


def build_scorer_driver():
    import kaldi_lstm_amd as k
    lib = k.lib_path()
    assert os.path.exists(lib), "libklstm.so missing: run __graft_entry__.build()"
    stale = (not os.path.exists(EXE)) or any(os.path.getmtime(f) > os.path.getmtime(EXE) for f in [SRC] + HDRS)
    if stale:
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), SRC,
                               "-L" + os.path.dirname(lib), "-lklstm", "-Wl,-rpath,$ORIGIN/../../kaldi-lstm_amd", "-o", EXE])
    return EXE


def run(*args, ok=True):
    r = subprocess.run([build_scorer_driver()] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    if ok:
        assert r.returncode == 0, r.stdout + r.stderr
    return r


I, C, R, NPDF = 8, 16, 8, 11


def dyadic(rng, shape, scale=64):
    """values that print the same at 6 digits (Kaldi's text precision) and at %.9g: text files compare byte for byte"""
    return (rng.randint(-scale, scale + 1, size=shape) / float(scale)).astype(np.float32)


def google_and_standard(shift, seed=0, two_layers=False):
    rng = np.random.RandomState(seed)
    n1 = 4 * C * I + 4 * C * R + 4 * C + 3 * C + R * C
    n2 = 4 * C * R + 4 * C * R + 4 * C + 3 * C + R * C
    f1, f2 = dyadic(rng, n1), dyadic(rng, n2)
    W, b = dyadic(rng, (NPDF, R)), dyadic(rng, NPDF)
    lstm_g = [("lstm_streams", f1, I, C, R, 4)] + ([("lstm_streams", f2, R, C, R, 4)] if two_layers else [])
    lstm_s = [("lstm", f1, I, C, R)] + ([("lstm", f2, R, C, R)] if two_layers else [])
    tail = [("affine", W, b), ("softmax", NPDF)]
    return [("transmit", I)] + lstm_g + tail, [("timeshift", I, shift)] + lstm_s + tail


@pytest.mark.parametrize("two_layers", [False, True])
@pytest.mark.parametrize("shift", [5, 0, -2])
def test_convert_to_standard_is_faq_q1(tmp_path, shift, two_layers):
    google, standard = google_and_standard(shift, seed=3 + shift, two_layers=two_layers)
    (tmp_path / "g.bin").write_bytes(kaldi_fmt.nnet_binary(google))
    out = run("convert", tmp_path / "g.bin", shift, 1, tmp_path / "s.bin").stdout.split()
    assert out == ["OK", str(len(standard)), "<TimeShift>"] + ["<LstmProjected>"] * (2 if two_layers else 1) + ["<AffineTransform>", "<Softmax>"]
    assert (tmp_path / "s.bin").read_bytes() == kaldi_fmt.nnet_binary(standard)          # binary: byte-identical
    run("convert", tmp_path / "g.bin", shift, 0, tmp_path / "s.txt")
    assert (tmp_path / "s.txt").read_bytes() == kaldi_fmt.nnet_text(standard)            # text: byte-identical
    (tmp_path / "g.txt").write_bytes(kaldi_fmt.nnet_text(google))                          # a text google model converts the same
    run("convert", tmp_path / "g.txt", shift, 1, tmp_path / "s2.bin")
    assert (tmp_path / "s2.bin").read_bytes() == kaldi_fmt.nnet_binary(standard)


def test_convert_refuses_what_has_no_standard_form(tmp_path):
    _, standard = google_and_standard(2)
    (tmp_path / "s.bin").write_bytes(kaldi_fmt.nnet_binary(standard))                      # already standard: a <TimeShift> in it
    r = run("convert", tmp_path / "s.bin", 2, 1, tmp_path / "x.bin", ok=False)
    assert r.returncode == 1 and "ERROR" in r.stdout and "<TimeShift>" in r.stdout
    assert not (tmp_path / "x.bin").exists()


def test_convert_refuses_a_model_without_transmit(tmp_path):
    google, _ = google_and_standard(3)
    (tmp_path / "g.bin").write_bytes(kaldi_fmt.nnet_binary(google[1:]))                    # LstmProjectedStreams first: no <Transmit>
    r = run("convert", tmp_path / "g.bin", 3, 1, tmp_path / "x.bin", ok=False)
    assert r.returncode == 1 and "<Transmit>" in r.stdout and "shift would be lost" in r.stdout
    assert not (tmp_path / "x.bin").exists()


def test_scorer_shift_resolution(tmp_path):
    google, standard = google_and_standard(4)
    (tmp_path / "g.bin").write_bytes(kaldi_fmt.nnet_binary(google))
    (tmp_path / "s.bin").write_bytes(kaldi_fmt.nnet_binary(standard))
    assert run("check", tmp_path / "s.bin", 16, 20, "loglike", "none").stdout.split() == ["OK", "shift", "4"]     # from the model
    assert run("check", tmp_path / "g.bin", 16, 20, "post", 5).stdout.split() == ["OK", "shift", "5"]            # from targets_delay
    assert run("check", tmp_path / "g.bin", 4, 50, "logpost", "none").stdout.split() == ["OK", "shift", "0"]     # Transmit = identity
    r = run("check", tmp_path / "s.bin", 16, 20, "post", 5, ok=False)                                            # both: refused
    assert r.returncode == 1 and "targets_delay" in r.stdout and "ambiguous" in r.stdout


def _rand_lstm(rng, i):
    return make_params(i, C, R, scale=0.1, seed=int(rng.randint(1 << 20)))


@pytest.mark.parametrize("case", ["no_affine", "affine_first", "two_softmax", "timeshift_inside", "no_lstm", "transmit_inside"])
def test_scorer_refuses_unsupported_topologies(tmp_path, case):
    rng = np.random.RandomState(7)
    lstm = ("lstm_streams", _rand_lstm(rng, I), I, C, R, 2)
    lstm2 = ("lstm_streams", _rand_lstm(rng, R), R, C, R, 2)
    aff_r = ("affine", dyadic(rng, (NPDF, R)), dyadic(rng, NPDF))
    aff_i = ("affine", dyadic(rng, (R, I)), dyadic(rng, R))
    nets = {
        "no_affine": [("transmit", I), lstm, ("softmax", R)],
        "affine_first": [aff_i, ("lstm_streams", _rand_lstm(rng, R), R, C, R, 2), aff_r, ("softmax", NPDF)],
        "two_softmax": [("transmit", I), lstm, aff_r, ("softmax", NPDF), ("softmax", NPDF)],
        "timeshift_inside": [("transmit", I), lstm, ("timeshift", R, 1), lstm2, aff_r, ("softmax", NPDF)],
        "no_lstm": [("transmit", I), aff_i, ("softmax", R)],
        "transmit_inside": [("transmit", I), lstm, ("transmit", R), lstm2, aff_r],
    }
    (tmp_path / "n.bin").write_bytes(kaldi_fmt.nnet_binary(nets[case]))
    r = run("check", tmp_path / "n.bin", 4, 20, "post", "none", ok=False)
    assert r.returncode == 1 and "BatchScorer" in r.stdout and "component" in r.stdout, r.stdout


def test_scorer_refuses_bad_options(tmp_path):
    google, _ = google_and_standard(0)
    (tmp_path / "g.bin").write_bytes(kaldi_fmt.nnet_binary(google))
    for args in [(0, 20, "post"), (16, 0, "post"), (300, 20, "post"), (16, 20, "argmax")]:
        r = run("check", tmp_path / "g.bin", *args, "none", ok=False)
        assert r.returncode == 1 and "BatchScorer" in r.stdout, (args, r.stdout)


def plan_numpy(lens, S, T):
    """The chunk plan restated: streams take the next non-empty utterance at a chunk boundary once theirs is finished."""
    off = np.concatenate([[0], np.cumsum(lens)]).astype(int)
    queue = [u for u in range(len(lens)) if lens[u] > 0]
    utt, cur = [None] * S, [0] * S
    chunks = []
    while True:
        for s in range(S):
            if utt[s] is None or cur[s] >= lens[utt[s]]:
                utt[s] = queue.pop(0) if queue else None
                cur[s] = 0
        if all(u is None for u in utt):
            return chunks
        desc = np.zeros((S, 3), int)
        reset = np.ones(S, int)
        dst = -np.ones((T, S), int)
        for s in range(S):
            if utt[s] is None:
                continue
            u, n = utt[s], lens[utt[s]]
            desc[s] = (off[u], n, cur[s])
            reset[s] = int(cur[s] == 0)
            t = np.arange(T)
            dst[:, s] = np.where(cur[s] + t < n, off[u] + cur[s] + t, -1)
            cur[s] += T
        chunks.append((desc.ravel(), reset, dst.ravel()))


@pytest.mark.parametrize("S,T,lens", [
    (4, 20, [37, 5, 0, 61, 20, 19, 21, 3, 44]),      # ragged, one empty, some shorter than T
    (16, 20, [7, 30, 12]),                            # fewer utterances than streams
    (3, 8, [8, 16, 1, 1, 1, 9, 0, 0, 33]),            # exact multiples of T, single frames, trailing empties
    (1, 50, [120, 3, 77]),                            # one stream: the per-utterance layout
    (5, 7, []),                                       # nothing to do
])
def test_chunk_plan_matches_numpy(S, T, lens):
    out = run("plan", S, T, ",".join(map(str, lens)) or ",").stdout.splitlines()
    exp = plan_numpy(lens, S, T)
    assert out[0] == "chunks %d" % len(exp)
    for c, (desc, reset, dst) in enumerate(exp):
        got = [np.array(out[1 + 3 * c + k].split(), int) for k in range(3)]
        assert np.array_equal(got[0], desc) and np.array_equal(got[1], reset) and np.array_equal(got[2], dst)
    # every frame of every utterance is written exactly once
    if lens:
        dsts = np.concatenate([d for _, _, d in exp])
        written = np.sort(dsts[dsts >= 0])
        assert np.array_equal(written, np.arange(sum(lens)))
