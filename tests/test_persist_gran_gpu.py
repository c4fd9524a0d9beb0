"""Engine option "persist_gran": what the in-launch exchange of the fp32 persistent forward chain carries at 1..4 streams.

0: {tag, value} granules of 8 bytes.  1 (default): value-only granules -- the 16 bytes of a cell's four stream values, fresh when a dword
differs from the signalling-NaN pattern its slot held before; one slot per step in one of two rings, the other ring handed back as that
pattern by every launch (the backward chain keeps the tags under either setting).  Only the transport differs: every result must be
BYTE-identical on twin engines, and the counters must show which transport ran (klstm_profile_query "gran_value_launches").

Shapes: 8/64/32 -- 16 chain workgroups and two 32-cell tail slots, the smallest geometry the chains take -- and one case at the headline
shape 40/800/512.  Frames per minibatch 8 / 9 / 20 (even and odd counts, both rings used three times in six minibatches), 40 (the rings
grow from 32 to 64 slots), 255 (above the cap of 254: that minibatch keeps the tags, the next one is value-only again).
"""
import numpy as np
import pytest
import torch

from oracle.oracle import make_params

pytestmark = pytest.mark.gpu

I, C, R = 8, 64, 32
T_CAP = 254                      # klstm_kernels.h GRAN_CAP_SLOTS - 2
EVENTS = ("persist_giveups", "persist_replayed", "persist_dropped")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b, what):
    assert a.keys() == b.keys()
    for key in a:
        assert a[key].shape == b[key].shape and np.array_equal(_bits(a[key]), _bits(b[key])), f"{what}: {key} is not byte-identical"


class _Run:
    """One engine with its own output buffers; counts what it expects of the launch counters as it goes."""

    def __init__(self, k, dims, S, p, persist, gran, stream=None, opts=None):
        self.I, self.C, self.R = dims
        self.e = k.Engine(self.I, self.C, self.R, S, stream=stream)
        self.e.set_params(p)
        self.e.set_option("persist", persist)
        self.e.set_option("persist_gran", gran)
        for key, v in (opts or {}).items():
            self.e.set_option(key, v)
        self.S, self.persist, self.gran = S, persist, gran
        self.graph = 0
        self.buf = {}
        self.want_value = 0          # launches that must have used the value-only transport
        self.want_launches = 0       # persistent launches in all

    def _bufs(self, T):
        if T not in self.buf:
            self.buf[T] = (torch.empty(T * self.S, self.R, device="cuda"), torch.empty(T * self.S, self.I, device="cuda"))
        return self.buf[T]

    def _count(self, T, directions):
        self.want_launches += directions
        if self.gran and not self.graph and T <= T_CAP:
            self.want_value += 1                      # (the forward launch)

    def set_graph(self, v):
        self.e.set_option("graph", v)
        self.graph = v

    def infer(self, x):
        T = x.shape[0] // self.S
        out = torch.empty(T * self.S, self.R, device="cuda")
        self.e.propagate_inference(x, out)
        self.e.synchronize()
        self._count(T, 1)
        return out.cpu().numpy()

    def step(self, x, od, planes=True):
        T = x.shape[0] // self.S
        out, idf = self._bufs(T)
        e = self.e
        e.propagate(x, out); e.backpropagate(x, od, idf, momentum=0.9, flags=2); e.update(1e-3)
        e.synchronize()
        self._count(T, 2 if self.persist == 2 else 1)
        c, r = e.get_state()
        res = dict(out=out.cpu().numpy(), in_diff=idf.cpu().numpy(), params=e.get_params(), corr=e.get_corr(), c=c, r=r)
        if planes:
            res.update(fwd_planes=e.activations(0), bwd_planes=e.activations(1))
        return res

    def check_counters(self):
        q = lambda name: self.e.profile_query(name)[1]
        for name in EVENTS:
            assert q(name) == 0, name                          # (nothing waited: no give-up on either transport)
        assert q("persist_launches") == self.want_launches > 0
        assert q("gran_value_launches") == self.want_value
        if self.gran:
            assert self.want_value > 0
        self.e.close()


def _mb(rng, T, S, dims=(I, C, R)):
    return (torch.from_numpy(rng.randn(T * S, dims[0]).astype(np.float32)).cuda(),
            torch.from_numpy(rng.randn(T * S, dims[2]).astype(np.float32)).cuda())


def _twins(k, S, persist=2, dims=(I, C, R), stream=None, opts=None, seed=5):
    p = make_params(*dims, scale=0.2, seed=seed)
    return [_Run(k, dims, S, p, persist, gran, stream=stream, opts=opts) for gran in (1, 0)]


@pytest.mark.parametrize("persist", [1, 2])
@pytest.mark.parametrize("T", [8, 9, 20])
@pytest.mark.parametrize("S", [1, 2, 3, 4])
def test_value_only_granules_are_byte_identical_to_tagged_ones(S, T, persist):
    """Six chained minibatches: both rings are used three times; S < 4 leaves dead stream dwords in every unit."""
    import kaldi_lstm_amd as k
    rng = np.random.RandomState(100 * S + T)
    a, b = _twins(k, S, persist)
    for i in range(6):
        x, od = _mb(rng, T, S)
        _same(a.step(x, od), b.step(x, od), f"minibatch {i}")
    a.check_counters(); b.check_counters()


@pytest.mark.parametrize("S", [3, 4])
def test_frames_per_minibatch_change_grow_the_rings_and_cross_the_cap(S):
    """T changes from minibatch to minibatch: the slots a launch poisons (what the other ring's last user wrote) differ from the slots it
    uses; T = 40 re-allocates the rings (32 -> 64 slots); T = 255 is above the cap: that minibatch runs on tags, the next ones on values
    again with the rings as the last value-only launches left them.  Reset flags in the middle of the run."""
    import kaldi_lstm_amd as k
    rng = np.random.RandomState(7 + S)
    a, b = _twins(k, S)
    for i, T in enumerate((20, 8, 20, 9, 40, 8, 255, 20, 9, 20)):
        if i in (3, 7):
            fl = np.zeros(S, np.int32); fl[::2] = 1
            a.e.reset(fl); b.e.reset(fl)
        x, od = _mb(rng, T, S)
        _same(a.step(x, od, planes=T < 100), b.step(x, od, planes=T < 100), f"minibatch {i} (T = {T})")
    assert a.want_value == 9                          # (every minibatch but the one above the cap)
    a.check_counters(); b.check_counters()


def test_graph_on_and_off_and_forward_only_calls_in_between():
    """"graph" 0 -> 2 -> 0: captured launches keep the tags (their own buffers: nothing to hand over); forward-only calls between
    training calls take a ring like any other forward launch."""
    import kaldi_lstm_amd as k
    S = 4
    rng = np.random.RandomState(3)
    a, b = _twins(k, S)
    xi = torch.from_numpy(rng.randn(7 * S, I).astype(np.float32)).cuda()
    mbs = [_mb(rng, T, S) for T in (20, 9)]           # (a cached graph holds the pointers it was captured with: two buffer sets)
    for i in range(10):
        if i == 3:
            a.set_graph(2); b.set_graph(2)
        if i == 6:
            a.set_graph(0); b.set_graph(0)
        if i in (1, 2, 4, 8):
            assert np.array_equal(_bits(a.infer(xi)), _bits(b.infer(xi))), f"forward-only call in front of minibatch {i}"
        x, od = mbs[i % 2]
        _same(a.step(x, od), b.step(x, od), f"minibatch {i}")
    assert 0 < a.want_value < a.want_launches
    a.check_counters(); b.check_counters()


def test_two_engines_on_one_stream():
    import kaldi_lstm_amd as k
    S = 4
    rng = np.random.RandomState(4)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        a0, b0 = _twins(k, S, stream=stream, seed=5)
        a1, b1 = _twins(k, S, stream=stream, seed=6)
        for i, T in enumerate((20, 9, 8, 20)):
            x, od = _mb(rng, T, S)
            ra0 = a0.step(x, od); ra1 = a1.step(x, od)          # (two value-only engines back to back on the stream)
            _same(ra0, b0.step(x, od), f"minibatch {i}, first engine")
            _same(ra1, b1.step(x, od), f"minibatch {i}, second engine")
    for r in (a0, b0, a1, b1):
        r.check_counters()


def test_a_quiet_nan_in_the_features_travels_like_any_value():
    """A quiet NaN differs from the poison pattern: the dwords it reaches count as fresh, nothing waits (no give-up), and the bytes are
    those of the tagged transport."""
    import kaldi_lstm_amd as k
    S = 4
    rng = np.random.RandomState(9)
    a, b = _twins(k, S)
    for i in range(3):
        x, od = _mb(rng, 9, S)
        if i == 1:
            x[2 * S + 1, :] = float("nan")            # (frame 3, stream 1)
        ra, rb = a.step(x, od), b.step(x, od)
        _same(ra, rb, f"minibatch {i}")
        if i == 1:
            assert np.isnan(ra["out"]).any()
    a.check_counters(); b.check_counters()


@pytest.mark.parametrize("tail", [1, 2])
def test_headline_shape(tail):
    """40/800/512, 4 streams, T = 20: 200 chain workgroups, two cells per sweeper thread; with the backward launch's d_r / in_diff on tail
    workgroups ("persist_tail" 1) and on the chain's own (2)."""
    import kaldi_lstm_amd as k
    dims, S, T = (40, 800, 512), 4, 20
    rng = np.random.RandomState(12)
    a, b = _twins(k, S, dims=dims, opts={"persist_tail": tail})
    for i in range(3):
        x, od = _mb(rng, T, S, dims)
        _same(a.step(x, od), b.step(x, od), f"minibatch {i}")
    tw = a.e.profile_query("persist_tail_wgs")[1]
    assert (tw > 0) == (tail == 1)
    a.check_counters(); b.check_counters()
