"""int8-quantized all-gather on one MI355X: the segmented dequantize kernels
of csrc/hip/kernels.hip bit for bit against the numpy reference and the host
twin, and the collective with every rank on device 0 (IPC window transport:
fused and wait-flag paths, several sub-messages per segment, staged pageable
buffers in accumulate mode, ShardedOptimizer(ag_compression="int8")).

Expectations, cases and rank workers live in tests/workers_quant_ag.py; the
host twin of this file is tests/test_quant_ag_cpu.py.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import quant_ref as qr  # noqa: E402
from tests import workers_quant_rs as w  # noqa: E402
from tests import workers_quant_ag as wa  # noqa: E402

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

SENTINEL = 0xCD
GUARD = qr.GUARD


def _gpu_dequantize_segments(wire, nseg, count, block, dtype, accumulate, offset_elems=0,
                             wire_front=0):
    """ops.dequantize_segments into a guarded buffer; returns out's bits.
    Allocations are 16-byte aligned and the guard in front of `out` is 64
    bytes, so `out` is 16-byte aligned exactly when offset_elems is 0; the
    wire starts `wire_front` bytes into its allocation and has sentinels
    around it. `out` starts as wa.kernel_base when accumulating and as 0xAB
    bytes otherwise."""
    from mlsl_amd import ops
    front = GUARD + offset_elems * w.ITEM[dtype]
    nbytes = nseg * count * w.ITEM[dtype]
    host_out = np.full(front + nbytes + GUARD, SENTINEL, dtype=np.uint8)
    host_out[front:front + nbytes] = (wa.kernel_base(nseg, count, dtype).view(np.uint8)
                                      if accumulate else 0xAB)
    d_out = torch.from_numpy(host_out).cuda()
    assert d_out.data_ptr() % 16 == 0
    h = np.full(wire_front + wire.size + GUARD, SENTINEL, dtype=np.uint8)
    h[wire_front:wire_front + wire.size] = wire
    d_wire = torch.from_numpy(h).cuda()
    assert d_wire.data_ptr() % 16 == 0
    ops.dequantize_segments(d_wire[wire_front:wire_front + wire.size],
                            d_out[front:front + nbytes], count, nseg, block=block,
                            dtype=dtype, accumulate=accumulate)
    torch.cuda.synchronize()
    assert np.array_equal(d_wire.cpu().numpy(), h), "wire modified, or a write around it"
    got = d_out.cpu().numpy()
    assert (got[:front] == SENTINEL).all() and (got[front + nbytes:] == SENTINEL).all(), \
        "write outside out"
    return got[front:front + nbytes].view(w.BITS[dtype]).copy()


@requires_gpu
class TestDequantizeSegments:
    def setup_method(self, _):
        torch.cuda.set_device(0)

    # offset 0: fast path where block == 256 and the count is whole blocks,
    # generic kernel otherwise, with misaligned segments 1.. at (1003, 128)
    # f32 and (1000, 256) bf16; offset 1: generic kernel, scalar stores
    @pytest.mark.parametrize("count,block,offset,nseg,accumulate,dtype", wa.KERNEL_PARAMS)
    def test_bits(self, count, block, offset, nseg, accumulate, dtype):
        wire = wa.kernel_wire(nseg, count, block)
        got = _gpu_dequantize_segments(wire, nseg, count, block, dtype, accumulate, offset)
        want = wa.kernel_expectation(nseg, count, block, dtype, accumulate)
        bad = int((got != want).sum())
        assert bad == 0, f"{bad} of {nseg * count} elements differ from the reference"
        assert np.array_equal(got, wa.host_dequantize_segments(
            wire, nseg, count, block, dtype, accumulate, offset)), "host twin differs"

    @pytest.mark.parametrize("accumulate", [False, True])
    @pytest.mark.parametrize("dtype", ["f32", "bf16"])
    def test_wire_at_8_byte_offset(self, dtype, accumulate):
        # a chunk's wire is 16-byte aligned, but the fast path must not need
        # that: it reads 8-byte payload words
        count, block, nseg = 1280, 256, 3
        wire = wa.kernel_wire(nseg, count, block)
        got = _gpu_dequantize_segments(wire, nseg, count, block, dtype, accumulate,
                                       wire_front=8)
        assert np.array_equal(got, wa.kernel_expectation(nseg, count, block, dtype,
                                                         accumulate))

    @pytest.mark.parametrize("dtype", ["f32", "bf16"])
    @pytest.mark.parametrize("count,block", [(1003, 128), (1280, 256)])
    def test_assign_is_dequantize_per_segment(self, count, block, dtype):
        from mlsl_amd import ops
        nseg = 3
        wire = wa.kernel_wire(nseg, count, block)
        got = _gpu_dequantize_segments(wire, nseg, count, block, dtype, False)
        seg_wire = qr.wire_bytes(count, block)
        d_wire = torch.from_numpy(np.array(wire)).cuda()
        for j in range(nseg):
            out = torch.zeros(count * w.ITEM[dtype], dtype=torch.uint8, device="cuda")
            ops.dequantize(d_wire[j * seg_wire:(j + 1) * seg_wire], out, count, block=block,
                           dtype=dtype)
            torch.cuda.synchronize()
            assert np.array_equal(got[j * count:(j + 1) * count],
                                  out.cpu().numpy().view(w.BITS[dtype])), j

    @pytest.mark.parametrize("dtype", ["f32", "bf16"])
    def test_flat_dequantize_is_wrong_for_partial_blocks(self, dtype):
        # the test cannot pass on a flat shortcut: see the host twin
        from mlsl_amd import ops
        count, block, nseg = 1003, 128, 3
        wire = wa.kernel_wire(nseg, count, block)
        want = wa.kernel_expectation(nseg, count, block, dtype, False)
        flat = torch.zeros(nseg * count * w.ITEM[dtype], dtype=torch.uint8, device="cuda")
        ops.dequantize(torch.from_numpy(np.array(wire)).cuda(), flat, nseg * count,
                       block=block, dtype=dtype)
        torch.cuda.synchronize()
        flat = flat.cpu().numpy().view(w.BITS[dtype])
        assert np.array_equal(flat[:count], want[:count])
        assert (flat[count:] != want[count:]).sum() > count
        got = _gpu_dequantize_segments(wire, nseg, count, block, dtype, False)
        assert np.array_equal(got, want)

    def test_rejects(self):
        from mlsl_amd import ops
        wire = torch.from_numpy(np.array(wa.kernel_wire(3, 20, 8))).cuda()
        out = torch.full((60,), 7.0, dtype=torch.float64, device="cuda")
        out32 = torch.full((60,), 7.0, dtype=torch.float32, device="cuda")
        with pytest.raises(RuntimeError, match="f32/bf16 only"):
            ops.dequantize_segments(wire, out, 20, 3, block=8, dtype="f64")
        with pytest.raises(RuntimeError, match="at least one segment"):
            ops.dequantize_segments(wire, out32, 20, 0, block=8)
        with pytest.raises(RuntimeError, match="multiple of 4"):
            ops.dequantize_segments(wire, out32, 20, 3, block=6, accumulate=True)
        torch.cuda.synchronize()
        assert (out == 7.0).all() and (out32 == 7.0).all(), "a rejected call wrote to out"


# ---- collective, every rank on device 0 ------------------------------------

@requires_gpu
@pytest.mark.parametrize("world", [1, 2, 4])   # 1: the n=1 branch, finish only
def test_quantized_all_gather(world):
    wa.assert_one_digest(wa.run_ranks("ag_check", world, device=True), world)


@requires_gpu
def test_quantized_all_gather_unfused_transport():
    # fused kernels off: wait-flag kernel, wide copy, set-flag kernel
    wa.run_ranks("ag_check", 2, device=True, extra_env={"MLSL_P2P_FUSED_MAX_KB": "0"})


@requires_gpu
def test_quantized_all_gather_multislot():
    # 1 MiB slots against a 3.1 MiB wire segment: several sub-messages per
    # segment, slot wrap, sub-message boundaries on wire-unit boundaries
    wa.run_ranks("ag_check", 2, device=True, extra_env={"MLSL_P2P_SLOT_MB": "1"},
                 shapes=[(3 << 20, 256)], dtypes=["f32"])


@requires_gpu
def test_quantized_all_gather_numpy_buffers_accumulate():
    # pageable send and recv buffers, accumulate mode: recv is an input of
    # the finish and has to be staged into HBM before it, then copied out
    wa.run_ranks("ag_check", 2, device="numpy", modes=["accumulate"], inplace=[False])


@requires_gpu
def test_sharded_optimizer_int8_all_gather():
    wa.run_ranks("ag_sharded_optimizer", 2, device=True)
