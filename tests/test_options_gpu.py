"""klstm_set_option as a table (csrc/klstm_engine.hip g_options): every key the strcmp chain took is still taken, unknown keys are
refused with the same text, what a key validates or clamps is validated and clamped as before, and setting every key to its default
changes nothing a minibatch computes.

One small engine shape throughout: I = 16, C = 32, R = 16, 2 streams, T = 3.  The keys that force a stall or a give-up are only SET here
(to 0); what they do is the subject of tests/test_persist_robustness_gpu.py.
"""
import numpy as np
import pytest
import torch

from oracle.oracle import make_params

pytestmark = pytest.mark.gpu

I, C, R, S, T = 16, 32, 16, 2, 3


def _defaults():
    """every key of the chain this table replaced, in the table's order, with the value a fresh engine has"""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    return [("graph", 0), ("vector", 1), ("small_max", 16), ("fat", 1), ("bf16", 0), ("d2h_small", 1), ("fat_fine", -1), ("small_nt2", -1),
            ("fuse_update", 1), ("gemm_copies_plan", 0), ("gemm_copies", 1), ("gemm_nt2", 1), ("fold", -1),
            ("persist", -1), ("persist_tpw", 0), ("persist_waves", 0), ("persist_bwd_waves", 0), ("persist_bwd_interleave", -1),
            ("persist_fwd_interleave", -1), ("persist_xl", -1), ("persist_xl_bwd", -1), ("persist_nap0", -1), ("persist_nap", -1),
            ("persist_nap0_bwd", -1), ("persist_spin_us", 50000), ("persist_test_stall_fwd", 0), ("persist_test_stall_bwd", 0),
            ("persist_ncu", ncu), ("persist_verify", 0), ("persist_verify_spin", 1), ("persist_epoch", 1), ("persist_gran", 1),
            ("persist_cooldown", 64), ("tail_merge", 0), ("persist_tail", 1),
            ("direct_nt_shape", 21), ("skinny_f16_pair", 1), ("skinny_f16", 1), ("outer_f16", 1), ("fold_direct", 1),
            ("fold_bf16x3", 2), ("fp16_products", 1), ("fuse_x", -1), ("profile", 0)]


@pytest.fixture(scope="module")
def k():
    import kaldi_lstm_amd as k
    return k


@pytest.fixture(scope="module")
def data():
    rng = np.random.RandomState(7)
    p = make_params(I, C, R, seed=3)
    x = torch.from_numpy(rng.randn(T * S, I).astype(np.float32)).cuda()
    od = torch.from_numpy(rng.randn(T * S, R).astype(np.float32)).cuda()
    return p, x, od


def _engine(k, p, i=I):
    e = k.Engine(i, C, R, S)
    if p is not None:
        e.set_params(p)
    return e


def _minibatch(e, x, od):
    out, idf = torch.empty(T * S, R, device="cuda"), torch.empty(T * S, I, device="cuda")
    e.propagate(x, out)
    e.backpropagate(x, od, idf, momentum=0.9)
    grads = e.get_grads()
    e.update(1e-2)
    e.synchronize()
    return dict(out=out.cpu().numpy(), in_diff=idf.cpu().numpy(), grads=grads, params=e.get_params(), corr=e.get_corr())


def _same(a, b, what):
    for key in a:
        assert np.array_equal(a[key], b[key]), f"{what}: {key} is not bit-identical"


def test_every_key_is_accepted_and_unknown_keys_are_refused(k, data):
    keys = _defaults()
    assert len(keys) == 44 and len({key for key, _ in keys}) == 44
    e = _engine(k, data[0])
    for key, v in keys:
        e.set_option(key, v)                         # (raises on any status but KLSTM_OK)
    for key in ("no_such_key", "persist_no_such"):
        with pytest.raises(k.KlstmError) as ei:
            e.set_option(key, 0)
        assert ei.value.status == 1 and f"klstm_set_option: unknown key '{key}'" in str(ei.value)


def test_validation_and_clamping_are_preserved(k, data):
    p, x, od = data
    e = _engine(k, p)
    with pytest.raises(k.KlstmError) as ei:
        e.set_option("gemm_copies_plan", 3)
    assert "gemm_copies_plan: 16 nj + ks with nj in {1, 2, 4} and ks in {1, 2, 4, 8} (or 0)" in str(ei.value)
    e.set_option("gemm_copies_plan", 16 * 2 + 4)
    e.set_option("gemm_copies_plan", 0)
    e12 = _engine(k, None, i=12)
    with pytest.raises(k.KlstmError) as ei:
        e12.set_option("bf16", 1)
    assert ei.value.status == 2 and "bf16 mode needs I, C, R multiples of 8" in str(ei.value)
    e12.set_option("bf16", 0)                        # taken on any shape; this one has no packed operands, so nothing is launched
    e12.synchronize()
    e.set_option("bf16", 1)                          # 2 streams: served by the fp32 chain, and the remark says so
    assert b"bf16 operand mode at 2 streams: served by the fp32 weights-resident chain" in e.lib.klstm_last_error()
    e.set_option("persist_cooldown", -5)             # (taken as 0: nothing here reads it back)
    e.set_option("fold_bf16x3", 9)                   # taken as 2, the default: the fold product's format as it runs says so
    assert e.profile_query("fold_mode")[1] == 2
    e.set_option("fold_bf16x3", -3)
    assert e.profile_query("fold_mode")[1] == 0


def test_graph_7_is_graph_2(k, data):
    """"graph" is clamped to 0..2.  2 differs from 1 in one place: a forward pass that is ONE persistent launch is captured into a graph
    too, and a captured launch keeps the tagged granules (klstm_profile_query "gran_value_launches" stays 0).  "persist" = 1 puts the
    three frames on that launch."""
    p, x, od = data
    seen = {}
    for g in (1, 2, 7):
        e = _engine(k, p)
        e.set_option("persist", 1)
        e.set_option("graph", g)
        out = torch.empty(T * S, R, device="cuda")
        e.propagate(x, out)
        e.synchronize()
        seen[g] = (out.cpu().numpy(), e.profile_query("persist_launches")[1], e.profile_query("gran_value_launches")[1])
        print("graph", g, "persist_launches", seen[g][1], "gran_value_launches", seen[g][2])
    assert np.array_equal(seen[7][0], seen[2][0]) and np.array_equal(seen[1][0], seen[2][0])
    assert seen[1][1:] == (1, 1), "the shape does not take the one-launch forward chain: the test cannot tell 2 from 1"
    assert seen[2][1:] == (1, 0) and seen[7][1:] == (1, 0)


def test_every_default_set_explicitly_changes_nothing(k, data):
    p, x, od = data
    fresh = _minibatch(_engine(k, p), x, od)
    e = _engine(k, p)
    for key, v in _defaults():
        e.set_option(key, v)
    _same(_minibatch(e, x, od), fresh, "all keys set to their defaults")
