"""Two-shot int8 allreduce on one MI355X: the N-way sum-requantize kernels of
csrc/hip/kernels.hip bit for bit against the numpy reference and the host
twin, out of place and in place, and the collective with every rank on
device 0 (IPC window transport: fused and wait-flag paths, several
sub-messages per range, pageable buffers, the n=1 branch).

Expectations, cases and rank workers live in tests/workers_quant_ar.py; the
host twin of this file is tests/test_quant_ar_cpu.py.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import workers_quant_ar as wa  # noqa: E402

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")


def _to_dev(host):
    d = torch.from_numpy(host).cuda()
    # 16-byte aligned allocations: a wire WIRE_FRONT = 8 bytes in is 8 but
    # not 16 bytes aligned
    assert d.data_ptr() % 16 == 0
    return d


def _to_host(d):
    torch.cuda.synchronize()
    return d.cpu().numpy()


def gpu_sum_requant_n(wires, nunits, block, alias=None):
    """ops.quant_sum_requant_n on guarded device buffers (sentinels around
    the destination and every wire; inputs compared with their originals);
    returns the destination's bytes."""
    from mlsl_amd import ops
    return wa.run_sum_requant_n(
        lambda ws, d, u, b: ops.quant_sum_requant_n(ws, d, u, block=b),
        _to_dev, _to_host, wires, nunits, block, alias)


@requires_gpu
class TestSumRequantN:
    def setup_method(self, _):
        torch.cuda.set_device(0)

    # block 256: the fast path (wires are 8-byte aligned); else the generic one
    @pytest.mark.parametrize("units,block,nwires", wa.KERNEL_PARAMS)
    def test_bits(self, units, block, nwires):
        wires = wa.kernel_wires(nwires, units, block)
        got = gpu_sum_requant_n(wires, units, block)
        want = wa.kernel_expectation(nwires, units, block)
        bad = int((got != want).sum())
        assert bad == 0, f"{bad} of {got.size} wire bytes differ from the reference"
        assert np.array_equal(got, wa.host_sum_requant_n(wires, units, block)), \
            "host twin differs"

    @pytest.mark.parametrize("units,block,nwires,k", wa.ALIAS_PARAMS)
    def test_in_place(self, units, block, nwires, k):
        # the destination IS wire k, as the schedule uses it: the out-of-place
        # bits, and no other wire touched
        wires = wa.kernel_wires(nwires, units, block)
        got = gpu_sum_requant_n(wires, units, block, alias=k)
        assert np.array_equal(got, wa.kernel_expectation(nwires, units, block))

    @pytest.mark.parametrize("block", [128, 256])
    def test_tie_and_zero_blocks(self, block):
        wa.check_constructed(gpu_sum_requant_n(wa.constructed_wires(block), 3, block), block)

    def test_generic_path_at_4_byte_alignment(self):
        # 256-blocks whose wires are only 4-byte aligned leave the fast path
        from mlsl_amd import ops
        units, block, nwires = 5, 256, 3
        wires = wa.kernel_wires(nwires, units, block)
        n = units * (block + 8)
        devs = [_to_dev(np.concatenate([np.zeros(4, np.uint8), x])) for x in wires]
        dst = _to_dev(np.full(4 + n + 12, wa.SENTINEL, dtype=np.uint8))
        ops.quant_sum_requant_n([d[4:4 + n] for d in devs], dst[4:4 + n], units, block=block)
        h = _to_host(dst)
        assert np.array_equal(h[4:4 + n], wa.kernel_expectation(nwires, units, block))
        assert (h[:4] == wa.SENTINEL).all() and (h[4 + n:] == wa.SENTINEL).all()

    def test_order_is_wire_order(self):
        got = wa.order_case(gpu_sum_requant_n)
        assert not np.array_equal(got[0], got[1])

    def test_rejects(self):
        from mlsl_amd import ops
        wires = [_to_dev(np.array(x)) for x in wa.kernel_wires(8, 3, 8)]
        dst = _to_dev(np.full(3 * 16, 0xAB, dtype=np.uint8))
        with pytest.raises(RuntimeError, match="1 to 8 wires"):
            ops.quant_sum_requant_n([], dst, 3, block=8)
        with pytest.raises(RuntimeError, match="1 to 8 wires"):
            ops.quant_sum_requant_n(wires + wires[:1], dst, 3, block=8)
        with pytest.raises(RuntimeError, match="multiple of 4"):
            ops.quant_sum_requant_n(wires, dst, 3, block=6)
        with pytest.raises(RuntimeError, match="multiple of 4"):
            ops.quant_sum_requant_n(wires, dst, 3, block=0)
        with pytest.raises(RuntimeError, match="4-byte aligned"):
            ops.quant_sum_requant_n([wires[0][2:]], dst, 1, block=8)
        # nothing was launched
        assert (_to_host(dst) == 0xAB).all()


# ---- collective, every rank on device 0 ------------------------------------

@requires_gpu
@pytest.mark.parametrize("world", [2, 4])
def test_twoshot_all_reduce(world):
    outs = wa.run_ranks("twoshot_check", world, device=True)
    wa.assert_ranks_agree(outs, world, configs=8)


@requires_gpu
def test_twoshot_all_reduce_unfused_transport():
    # fused kernels off: wait-flag kernel, wide copy, set-flag kernel
    outs = wa.run_ranks("twoshot_check", 2, device=True,
                        extra_env={"MLSL_P2P_FUSED_MAX_KB": "0"})
    wa.assert_ranks_agree(outs, 2, configs=8)


@requires_gpu
def test_twoshot_all_reduce_multislot():
    # 1 MiB slots against a 3.1 MiB range: several sub-messages per range in
    # both exchanges, slot wrap, sub-message boundaries on wire-unit boundaries
    outs = wa.run_ranks("twoshot_check", 2, device=True, extra_env={"MLSL_P2P_SLOT_MB": "1"},
                        shapes=[(6 << 20, 256)], dtypes=["f32"])
    wa.assert_ranks_agree(outs, 2, configs=2)


@requires_gpu
def test_twoshot_all_reduce_numpy_buffers():
    # pageable send and recv buffers: staged through HBM around the
    # compressed issue path, the pinned bounce copied out at completion
    outs = wa.run_ranks("twoshot_check", 2, device="numpy", inplace=[False])
    wa.assert_ranks_agree(outs, 2, configs=4)


@requires_gpu
def test_twoshot_all_reduce_single_rank():
    # n=1: quantize -> dequantize, exactly what the ring gives there
    wa.run_ranks("twoshot_check", 1, device=True)
    two = wa.digests(wa.run_ranks("digest_outputs", 1, device=True, ar_algo="two_shot"))
    ring = wa.digests(wa.run_ranks("digest_outputs", 1, device=True, ar_algo="ring"))
    assert two == ring and len(two[0]) == 8
