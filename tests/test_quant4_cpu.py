"""The int4 wire codec on the CPU: the host twins bit for bit against the numpy
reference (tests/quant4_ref.py), and the bits=4 collectives over TCP against
the host twins (tests/workers_quant4.py)."""
import numpy as np
import pytest

from tests import quant4_ref as q4
from tests import quant_ref as qr
from tests import workers_quant4 as w4
from tests import workers_quant_rs as w

NP_DT = w.NP_DT
# block 256 around the word (8) and block boundaries; blocks 8, 24 (20-byte wire
# blocks: every second one only 4-byte aligned) and 128 with make_input's tie,
# zero and negative-extreme blocks; five whole 256-blocks
CODEC_CASES = [(c, 256) for c in (1, 7, 8, 9, 255, 256, 257, 512)] + \
    [(61, 8), (100, 24), (1003, 128), (1280, 256)]


def host_codec(count, block, dtype, use_err):
    """Host twins against the reference; returns (inp, err before, reference)."""
    from mlsl_amd import ops
    inp, err0 = q4.make_input(count, block, dtype, seed=count + block)
    if use_err == "zero":
        err0 = np.zeros_like(err0)
    want = q4.codec(inp, None if use_err == "none" else err0, count, block, dtype)
    if use_err == "none":
        want["err"] = err0
    assert ops.wire_bytes(count, block, 4) == want["wire"].size
    wire_g, wire = qr.guarded(want["wire"].size, np.uint8, 0xAB)
    out_g, out = qr.guarded(count, NP_DT[dtype], 0xAB)
    err_g, err = qr.guarded(count, NP_DT[dtype], 0)
    err[:] = err0
    ops.host_quantize4(inp, wire, count, err=None if use_err == "none" else err, block=block,
                       dtype=dtype)
    ops.host_dequantize4(wire, out, count, block=block, dtype=dtype)
    assert np.array_equal(wire, want["wire"]), "wire (header, payload, zero padding)"
    assert np.array_equal(out, want["out"]) and np.array_equal(err, want["err"])
    assert all((g[-qr.GUARD:] == 0xCD).all() for g in (wire_g, out_g, err_g))
    if count >= 3 * block:
        s, word1, q = q4.unpack(wire, block)
        assert s[q4.TIE_BLOCK] == 0.125 and s[q4.ZERO_BLOCK] == 1.0 and not word1.any()
        assert q[q4.NEG_BLOCK, 0] == -7 and q.min() == -7 and q.max() == 7
    return inp, err0, want


def host_sums(count, block, nwires):
    """N-way host twins against the reference; returns (wires, {dtype: sum},
    requantized wire)."""
    from mlsl_amd import ops
    wires = q4.make_wires(nwires, count, block, seed=count + nwires)
    outs = {}
    for dtype in ("f32", "bf16"):
        outs[dtype] = q4.sum_dequant(wires, count, block, dtype)
        out = np.zeros(count, dtype=NP_DT[dtype])
        ops.host_quant_sum_dequant_n4(wires, out, count, block=block, dtype=dtype)
        assert np.array_equal(out, outs[dtype])
    want = q4.sum_requant(wires, block)
    for alias in (None, 0, nwires - 1):
        ws = [x.copy() for x in wires]
        dst = np.zeros_like(want) if alias is None else ws[alias]
        ops.host_quant_sum_requant_n4(ws, dst, qr.nblocks(count, block), block=block)
        assert np.array_equal(dst, want), f"dst is wire {alias}"
    if nwires >= 3 and count >= 1000:
        # from three wires on the order of the fma chain shows in the bits (two
        # wires round once either way), and the reference agrees
        out = np.zeros(count, dtype=np.float32)
        ops.host_quant_sum_dequant_n4(wires[::-1], out, count, block=block, dtype="f32")
        assert np.array_equal(out, q4.sum_dequant(wires[::-1], count, block, "f32"))
        assert not np.array_equal(out, outs["f32"])
    return wires, outs, want


@pytest.mark.parametrize("use_err", ["none", "zero", "rand"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("count,block", CODEC_CASES)
def test_host_codec(count, block, dtype, use_err):
    host_codec(count, block, dtype, use_err)


@pytest.mark.parametrize("nwires", [1, 2, 3, 8])
@pytest.mark.parametrize("count,block", [(61, 8), (100, 24), (1000, 256), (1280, 256)])
def test_host_sums(count, block, nwires):
    host_sums(count, block, nwires)


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("kind", ["all_reduce", "reduce_scatter"])
def test_collective_tcp(kind, world):
    w4.run_ranks("coll_check", world, kind=kind)


@pytest.mark.parametrize("world,plugin", [(1, True), (9, False)])
def test_refusals(world, plugin):
    if plugin:
        w.ensure_plugin()
    w4.run_ranks("refusals", world, plugin=plugin)


def test_sharded_optimizer_tcp():
    w4.run_ranks("sharded_optimizer", 2)
