"""One-shot (direct) int8 reduce-scatter on one MI355X: the N-way
sum-dequantize kernels of csrc/hip/kernels.hip bit for bit against the numpy
reference and the host twin, and the collective with every rank on device 0
(IPC window transport: fused and wait-flag paths, several sub-messages per
segment, ShardedOptimizer).

Expectations, cases and rank workers live in tests/workers_quant_rs_direct.py;
the host twin of this file is tests/test_quant_rs_direct_cpu.py.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import quant_ref as qr  # noqa: E402
from tests import workers_quant_rs as w  # noqa: E402
from tests import workers_quant_rs_direct as wd  # noqa: E402

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

SENTINEL = 0xCD
GUARD = qr.GUARD


def _gpu_sum_dequant_n(wires, count, block, dtype, offset_elems=0, wire_front=0):
    """ops.quant_sum_dequant_n into a guarded buffer; returns out's bits.
    Allocations are 16-byte aligned and the guard in front of `out` is 64
    bytes, so `out` is 16-byte aligned exactly when offset_elems is 0; every
    wire starts `wire_front` bytes into its allocation and has sentinels
    behind it."""
    from mlsl_amd import ops
    front = GUARD + offset_elems * w.ITEM[dtype]
    nbytes = count * w.ITEM[dtype]
    host_out = np.full(front + nbytes + GUARD, SENTINEL, dtype=np.uint8)
    host_out[front:front + nbytes] = 0xAB
    d_out = torch.from_numpy(host_out).cuda()
    assert d_out.data_ptr() % 16 == 0
    d_wires = []
    for x in wires:
        h = np.full(wire_front + x.size + GUARD, SENTINEL, dtype=np.uint8)
        h[wire_front:wire_front + x.size] = x
        d = torch.from_numpy(h).cuda()
        assert d.data_ptr() % 16 == 0
        d_wires.append(d)
    ops.quant_sum_dequant_n([d[wire_front:wire_front + x.size]
                             for d, x in zip(d_wires, wires)],
                            d_out[front:front + nbytes], count, block=block, dtype=dtype)
    torch.cuda.synchronize()
    for d, x in zip(d_wires, wires):
        h = d.cpu().numpy()
        assert np.array_equal(h[wire_front:wire_front + x.size], x), "wire modified"
        assert (h[:wire_front] == SENTINEL).all() and \
            (h[wire_front + x.size:] == SENTINEL).all(), "write around a wire"
    h = d_out.cpu().numpy()
    assert (h[:front] == SENTINEL).all() and (h[front + nbytes:] == SENTINEL).all(), \
        "write outside out"
    return h[front:front + nbytes].view(w.BITS[dtype]).copy()


@requires_gpu
class TestSumDequantN:
    def setup_method(self, _):
        torch.cuda.set_device(0)

    # offset 0: fast path where block == 256 and the count is whole blocks,
    # generic kernel otherwise; offset 1: generic kernel, scalar stores
    @pytest.mark.parametrize("count,block,offset,nwires,dtype", wd.KERNEL_PARAMS)
    def test_bits(self, count, block, offset, nwires, dtype):
        wires = wd.kernel_wires(nwires, count, block)
        got = _gpu_sum_dequant_n(wires, count, block, dtype, offset)
        want = wd.kernel_expectation(nwires, count, block, dtype)
        bad = int((got != want).sum())
        assert bad == 0, f"{bad} of {count} elements differ from the reference"
        assert np.array_equal(got, wd.host_sum_dequant_n(wires, count, block, dtype,
                                                         offset)), "host twin differs"

    @pytest.mark.parametrize("dtype", ["f32", "bf16"])
    @pytest.mark.parametrize("nwires", wd.KERNEL_NWIRES)
    def test_wires_at_8_byte_offsets(self, nwires, dtype):
        # TMP slots and wire segments start at multiples of 264 bytes: the
        # fast path must take wires that are 8 but not 16 bytes aligned
        count, block = 1280, 256
        wires = wd.kernel_wires(nwires, count, block)
        got = _gpu_sum_dequant_n(wires, count, block, dtype, wire_front=8)
        assert np.array_equal(got, wd.kernel_expectation(nwires, count, block, dtype))

    def test_rejects(self):
        from mlsl_amd import ops
        wires = [torch.from_numpy(np.array(x)).cuda() for x in wd.kernel_wires(8, 20, 8)]
        out = torch.zeros(20, dtype=torch.float64, device="cuda")
        with pytest.raises(RuntimeError, match="f32/bf16 only"):
            ops.quant_sum_dequant_n(wires, out, 20, block=8, dtype="f64")
        out32 = torch.zeros(20, dtype=torch.float32, device="cuda")
        with pytest.raises(RuntimeError, match="1 to 8 wires"):
            ops.quant_sum_dequant_n([], out32, 20, block=8)
        with pytest.raises(RuntimeError, match="1 to 8 wires"):
            ops.quant_sum_dequant_n(wires + wires[:1], out32, 20, block=8)
        with pytest.raises(RuntimeError):
            ops.quant_sum_dequant_n(wires, out32, 20, block=6)
        torch.cuda.synchronize()
        assert (out32 == 0).all()


# ---- collective, every rank on device 0 ------------------------------------

@requires_gpu
@pytest.mark.parametrize("world", [2, 4])
def test_direct_reduce_scatter(world):
    wd.run_ranks("direct_check", world, device=True)


@requires_gpu
def test_direct_reduce_scatter_unfused_transport():
    # fused kernels off: wait-flag kernel, wide copy, set-flag kernel
    wd.run_ranks("direct_check", 2, device=True, extra_env={"MLSL_P2P_FUSED_MAX_KB": "0"})


@requires_gpu
def test_direct_reduce_scatter_multislot():
    # 1 MiB slots against a 3.1 MiB wire segment: several sub-messages per
    # segment, slot wrap, sub-message boundaries on wire-unit boundaries
    wd.run_ranks("direct_check", 2, device=True, extra_env={"MLSL_P2P_SLOT_MB": "1"},
                 shapes=[(3 << 20, 256)], dtypes=["f32"])


@requires_gpu
def test_direct_reduce_scatter_numpy_buffers():
    # pageable send and recv buffers: staged through HBM around the
    # compressed issue path, the pinned bounce copied out at completion
    wd.run_ranks("direct_check", 2, device="numpy", inplace=[False])


@requires_gpu
def test_sharded_optimizer_int8_direct():
    wd.run_ranks("direct_sharded_optimizer", 2, device=True)
