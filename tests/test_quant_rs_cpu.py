"""int8-quantized reduce-scatter on the host: the fused sum-dequantize of
csrc/comm/quant.cpp bit for bit, and the collective over the TCP transport
(per-segment block grid, fused last hop, error feedback, in-place shards).

Expectations, cases and rank workers live in tests/workers_quant_rs.py; the
GPU twin of this file is tests/test_gpu_quant_rs.py.
"""
import numpy as np
import pytest

from tests import quant_ref as qr
from tests import workers_quant_rs as w

SENTINEL = 0xCD
GUARD = qr.GUARD


def _host_sum_dequant(a, b, count, block, dtype, offset_elems=0):
    """ops.host_quant_sum_dequant into a guarded buffer; returns out's bits.
    Sentinels sit in front of and behind `out`; both wires are compared
    with their copies afterwards."""
    from mlsl_amd import ops
    front = GUARD + offset_elems * w.ITEM[dtype]
    nbytes = count * w.ITEM[dtype]
    whole = np.full(front + nbytes + GUARD, SENTINEL, dtype=np.uint8)
    whole[front:front + nbytes] = 0xAB
    out = whole[front:front + nbytes].view(w.NP_DT[dtype])
    a_in, b_in = a.copy(), b.copy()
    ops.host_quant_sum_dequant(a_in, b_in, out, count, block=block, dtype=dtype)
    assert np.array_equal(a_in, a) and np.array_equal(b_in, b), "wire modified"
    assert (whole[:front] == SENTINEL).all() and (whole[front + nbytes:] == SENTINEL).all(), \
        "write outside out"
    return out.view(w.BITS[dtype]).copy()


CASES = [(c, b, 0) for c, b in w.KERNEL_CASES] + [w.OFFSET_CASE + (1,)]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("count,block,offset", CASES)
def test_host_sum_dequant_exact_wires(count, block, offset, dtype):
    a, b, _ = qr.make_exact_wires(count, block, seed=count)
    got = _host_sum_dequant(a, b, count, block, dtype, offset)
    assert np.array_equal(got, w.exact_wire_sum(a, b, count, block, dtype))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("count,block,offset", CASES)
def test_host_sum_dequant_random_wires(count, block, offset, dtype):
    a, b = w.random_wires(count, block, seed=count)
    got = _host_sum_dequant(a, b, count, block, dtype, offset)
    ok = w.matches_a_candidate(got, w.sum_candidates(a, b, count, block, dtype))
    assert ok.all(), f"{(~ok).sum()} elements match no candidate"


def test_host_sum_dequant_rejects_other_dtypes_and_blocks():
    from mlsl_amd import ops
    from mlsl_amd._lib import check, lib
    a, b, _ = qr.make_exact_wires(64, 8, seed=1)
    out = np.zeros(64, dtype=np.float64)
    ops.host_quant_sum_dequant(a, b, out.view(np.float32), 64, block=8)  # declares
    with pytest.raises(RuntimeError, match="f32/bf16 only"):
        check(lib().mlsl_host_quant_sum_dequant(
            a.ctypes.data, b.ctypes.data, out.ctypes.data, 64, 8, ops.DTYPE["f64"]))
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.host_quant_sum_dequant(a, b, out.view(np.float32), 64, block=6)


# ---- collective, TCP host transport ----------------------------------------

@pytest.mark.parametrize("world", [2, 3, 4])
def test_quant_reduce_scatter(world):
    """World 2: bit check (fails where `quantized=True` is ignored: the
    exact sum is none of the candidates). Worlds 3 and 4: error bound."""
    w.run_ranks("rs_check", world)


def test_quant_reduce_scatter_error_feedback():
    w.run_ranks("rs_error_feedback", 2)


def test_sharded_optimizer_int8():
    w.run_ranks("rs_sharded_optimizer", 2)


@pytest.mark.parametrize("world", [2, 3])
def test_quant_reduce_scatter_plugin(world):
    w.ensure_plugin()
    w.run_ranks("rs_plugin", world)


@pytest.fixture
def world1(monkeypatch):
    monkeypatch.setenv("MLSL_TRANSPORT", "tcp")
    import mlsl_amd as mx
    mx.init()
    try:
        yield mx
    finally:
        mx.set_quant_params(256)
        mx.finalize()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("count,block", w.COLL_SHAPES)
def test_quant_reduce_scatter_world1(world1, count, block, dtype):
    mx = world1
    mx.set_quant_params(block)
    d = mx.Distribution(1, 1)
    x = w.rank_input(0, count, dtype)
    out = np.zeros_like(x)
    req = mx.PersistentRequest(d, "reduce_scatter", count, dtype=dtype, op="sum",
                               group="data", quantized=True)
    send = x.copy()
    req.start(send, out)
    req.wait()
    req.destroy()
    assert np.array_equal(send, x), "send buffer modified"
    want = qr.ref_dequantize(*qr.ref_quantize(qr.decode(x, dtype), block), count, dtype)
    assert np.array_equal(out.view(w.BITS[dtype]), want.view(w.BITS[dtype]))


def test_quantized_reduce_scatter_rejects(world1):
    mx = world1
    import torch
    from mlsl_amd.parallel.zero1 import ShardedOptimizer
    d = mx.Distribution(1, 1)
    with pytest.raises(RuntimeError, match="SUM"):
        mx.PersistentRequest(d, "reduce_scatter", 64, dtype="f32", op="max",
                             group="data", quantized=True)
    with pytest.raises(RuntimeError, match="f32/bf16"):
        mx.PersistentRequest(d, "reduce_scatter", 64, dtype="f64", op="sum",
                             group="data", quantized=True)
    params = [torch.nn.Parameter(torch.zeros(8))]
    with pytest.raises(ValueError):
        ShardedOptimizer(params, torch.optim.SGD, d, reduce="none",
                         compression="int8", lr=0.1)
    with pytest.raises(ValueError):
        ShardedOptimizer([torch.nn.Parameter(torch.zeros(8, dtype=torch.float64))],
                         torch.optim.SGD, d, reduce="rs", compression="int8", lr=0.1)
