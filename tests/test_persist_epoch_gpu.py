"""Engine option "persist_epoch": where a persistent launch takes its epoch and launch ordinal from, and how it ends.

1 (default): a launch that goes straight to the stream gets both as kernel arguments from the engine's host mirror, workgroup 0 writes the
device words' next values at the head of the launch, and the workgroups exit without counting themselves in unless the host waits on the
done word ("persist_verify").  0: the launch reads the device words and its last workgroup moves them on (what a launch captured into a
hipGraph always does).  Neither moves a byte of the exchange or changes an arithmetic instruction: results are BIT-IDENTICAL, the device
words end up the same, and an engine may switch between the two -- and between plain launches and graphs -- at any minibatch boundary.

Shapes: the smallest at which both chains run -- C = 64 gives 16 chain workgroups and two 32-cell tail slots; 1 / 4 / 5 / 8 streams = one
group, a full group, a ragged second group, two full groups (the interleaved kernels); frames per minibatch cycle through 20, 3, 7, 20, 2 so
that the epochs advance unevenly and one minibatch of the cycle (T = 2 < 3) is never enqueued on the persistent chain: the mirror must
not move for it.  "persist" = 1 forces the forward chain, 2 both chains (the backward epoch word then moves too).
"""
import numpy as np
import pytest
import torch

from oracle.oracle import make_params

pytestmark = pytest.mark.gpu

T_CYCLE = (20, 3, 7, 20, 2)
N_MB = 40
WORDS = ("persist_word_epoch_fwd", "persist_word_epoch_bwd", "persist_word_launches")
EVENTS = ("persist_giveups", "persist_replayed", "persist_dropped")


def _data(I, R, S, n, seed):
    rng = np.random.RandomState(seed)
    mbs = []
    for i in range(n):
        T = T_CYCLE[i % len(T_CYCLE)]
        mbs.append((T, torch.from_numpy(rng.randn(T * S, I).astype(np.float32)).cuda(),
                    torch.from_numpy(rng.randn(T * S, R).astype(np.float32)).cuda()))
    xi = torch.from_numpy(rng.randn(7 * S, I).astype(np.float32)).cuda()      # the one propagate_inference call
    return mbs, xi


class _Run:
    """One engine and its own output buffers (a cached graph holds the pointers it was captured with)."""

    def __init__(self, k, I, C, R, S, p, persist, opts):
        self.e = k.Engine(I, C, R, S)
        self.e.set_params(p)
        self.e.set_option("persist", persist)
        for key, v in opts.items():
            self.e.set_option(key, v)
        self.I, self.R, self.S = I, R, S
        self.out = {T: torch.empty(T * S, R, device="cuda") for T in set(T_CYCLE)}
        self.idf = {T: torch.empty(T * S, I, device="cuda") for T in set(T_CYCLE)}
        self.out_inf = torch.empty(7 * S, R, device="cuda")

    def step(self, i, mb, xi, reset_every=10, inf_at=17):
        T, x, od = mb
        e = self.e
        if i % reset_every == 0:
            fl = np.zeros(self.S, np.int32); fl[:: 2] = 1
            e.reset(fl)
        res = {}
        if i == inf_at:
            e.propagate_inference(xi, self.out_inf)
            e.synchronize()
            res["out_inf"] = self.out_inf.cpu().numpy()
        e.propagate(x, self.out[T]); e.backpropagate(x, od, self.idf[T], momentum=0.9, flags=2); e.update(1e-3)
        e.synchronize()
        res.update(out=self.out[T].cpu().numpy(), in_diff=self.idf[T].cpu().numpy(), params=e.get_params())
        return res


def _same(a, b, what):
    assert a.keys() == b.keys()
    for key in a:
        assert np.array_equal(a[key], b[key]), f"{what}: {key} is not bit-identical"


def _expected_words(S, persist, inf_at=17):
    """What the device words must hold after N_MB minibatches: every ENQUEUED persistent launch moved its direction's epoch on by its tag
    count (forward T + 2, backward T + 2 per group of 4 streams) and the launch count by one; T = 2 minibatches enqueue none."""
    fwd = bwd = n = 0
    for i in range(N_MB):
        T = T_CYCLE[i % len(T_CYCLE)]
        if i == inf_at:
            fwd += 7 + 2; n += 1
        if T >= 3:
            fwd += T + 2; n += 1
            if persist == 2:
                bwd += ((S + 3) // 4) * (T + 2); n += 1
    return fwd, bwd, n


@pytest.mark.parametrize("persist", [1, 2])
@pytest.mark.parametrize("S", [1, 4, 5, 8])
@pytest.mark.parametrize("I,C,R", [(40, 64, 32), (8, 64, 32)])
def test_host_epoch_device_epoch_and_switching_engines_agree_bit_for_bit(I, C, R, S, persist):
    import kaldi_lstm_amd as k
    p = make_params(I, C, R, scale=0.2, seed=5)
    mbs, xi = _data(I, R, S, N_MB, 11)
    runs = [_Run(k, I, C, R, S, p, persist, {"persist_epoch": 1}),
            _Run(k, I, C, R, S, p, persist, {"persist_epoch": 0}),
            _Run(k, I, C, R, S, p, persist, {})]                       # flips the option every 5 minibatches, graphs in the middle
    for i, mb in enumerate(mbs):
        if i % 5 == 0:
            runs[2].e.set_option("persist_epoch", (i // 5 + 1) % 2)
        if i == 13:
            runs[2].e.set_option("graph", 2)          # (a switch inside a stretch of "persist_epoch" = 1: captured launches read the device words)
        if i == 27:
            runs[2].e.set_option("graph", 0)
        got = [r.step(i, mb, xi) for r in runs]
        _same(got[0], got[1], f"minibatch {i} (T = {mb[0]}), persist_epoch 1 against 0")
        _same(got[0], got[2], f"minibatch {i} (T = {mb[0]}), persist_epoch 1 against the switching engine")
    want = _expected_words(S, persist)
    for r in runs:
        for name in EVENTS:
            assert r.e.profile_query(name)[1] == 0, name
        words = tuple(r.e.profile_query(name)[1] for name in WORDS)
        assert words == want                          # (the device words, read back: equal on the three engines and what was enqueued)
        assert r.e.profile_query("persist_launches")[1] == want[2] > 0   # (the host's count: the chain DID run)
        r.e.close()


@pytest.mark.parametrize("S", [4, 8])
def test_persist_verify_still_hears_the_done_word(S):
    """The host waits on the done word inside every call: the launches keep the arrival count and the last workgroup's report under
    either setting -- the calls return (a missing report would cost the one-second fall-back of every wait), bit-identical, no give-up."""
    import kaldi_lstm_amd as k
    I, C, R = 40, 64, 32
    p = make_params(I, C, R, scale=0.2, seed=5)
    mbs, xi = _data(I, R, S, 10, 11)
    runs = [_Run(k, I, C, R, S, p, 2, {"persist_verify": 1, "persist_epoch": pe}) for pe in (1, 0)]
    plain = _Run(k, I, C, R, S, p, 2, {})
    for i, mb in enumerate(mbs):
        got = [r.step(i, mb, xi, inf_at=3) for r in runs]
        _same(got[0], got[1], f"minibatch {i}, persist_verify with persist_epoch 1 against 0")
        _same(got[0], plain.step(i, mb, xi, inf_at=3), f"minibatch {i}, persist_verify against an engine that does not wait")
    for r in runs + [plain]:
        for name in EVENTS:
            assert r.e.profile_query(name)[1] == 0, name
        assert r.e.profile_query("persist_launches")[1] == r.e.profile_query("persist_word_launches")[1] > 0
        r.e.close()
