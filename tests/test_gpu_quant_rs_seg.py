"""The quantized reduce-scatter over a list of tensors on one MI355X: the
prologue kernel against the numpy reference, the flat quantize launched per
shard on the materialised, padded concatenation, and its host twin, bit for
bit; the request on one device (the n=1 branch, IPC windows at worlds 2 and 4)
against the flat quantized reduce_scatter; ShardedOptimizer(grads="in_place")
against grads="copy" on device tensors.

Kernel paths (csrc/hip/kernels.hip, QuantizeGatherShardsKernel): a block of
256 real elements inside one tensor, with its first element there and its
residual both 16-byte aligned, stays in registers; a block inside one tensor
at an aligned address takes the 4-wide loop; every other block walks; a block
of padding only reads nothing. Which one a block takes is decided per block:
with an odd shard, shard 1 of an "al16" case is misaligned throughout.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import quant_seg_ref as sr  # noqa: E402
from tests import workers_quant_rs_seg as wq  # noqa: E402

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")


class GpuApi:
    """The kernels on torch uint8 tensors of GPU 0."""

    def put(self, img):
        return torch.from_numpy(np.array(img, copy=True)).cuda()

    def get(self, buf):
        torch.cuda.synchronize()
        return buf.cpu().numpy()

    def quantize_gather_shards(self, tensors, counts, wire, nshards, shard, err, block, dtype,
                               wire_stride):
        from mlsl_amd import ops
        ops.quantize_gather_shards(tensors, counts, wire, nshards, shard, err=err, block=block,
                                   dtype=dtype, wire_stride=wire_stride)

    def quantize_gather(self, tensors, counts, wire, err, block, dtype):
        from mlsl_amd import ops
        ops.quantize_gather(tensors, counts, wire, err=err, block=block, dtype=dtype)

    def quantize(self, inp, wire, count, err, block, dtype):
        from mlsl_amd import ops
        ops.quantize(inp, wire, count, err=err, block=block, dtype=dtype)


def _against_host(case, wire_stride=None):
    gpu = wq.run_shard_case(GpuApi(), *case, wire_stride=wire_stride)
    host = wq.run_shard_case(wq.HostApi(), *case, wire_stride=wire_stride)
    assert np.array_equal(gpu["wire"], host["wire"]), "wire differs from the host twin's"
    # the residual is defined up to the fusion of v - q*scale (both runs were
    # checked against the two roundings): where the two forms agree, so must
    # the twins
    layout, n, shard, block, dtype, use_err, _ = case
    if use_err:
        same = wq.residual_forms_agree(layout, n, shard, block, dtype)
        assert np.array_equal(gpu["err"][same], host["err"][same])


@requires_gpu
class TestKernel:
    def setup_method(self, _):
        torch.cuda.set_device(0)

    @pytest.mark.parametrize("case", wq.SHARD_PARAMS, ids=wq.shard_id)
    def test_against_numpy_flat_and_host(self, case):
        _against_host(case)

    @pytest.mark.parametrize("dtype", ["f32", "bf16"])
    @pytest.mark.parametrize("case", wq.ODD_WIRE_SHARD_CASES, ids=str)
    def test_wire_of_4_mod_8_bytes(self, case, dtype):
        # blocks of 12 and 100 elements, an odd number per shard: the plan's
        # stride, one shard's wire exactly, is a multiple of 4 and not of 8
        layout, n, shard, block = case
        sw = sr.qr.wire_bytes(shard, block)
        assert sw % 8 == 4
        for misalign in (False, True):
            _against_host((layout, n, shard, block, dtype, True, misalign), wire_stride=sw)

    @pytest.mark.parametrize("extra", [0, 4, 8, 24])
    def test_wire_stride(self, extra):
        # the plan's stride is one shard's wire exactly
        stride = sr.qr.wire_bytes(513, 256) + extra
        _against_host(("edges", 4, 513, 256, "f32", True, True), wire_stride=stride)

    def test_tables_in_device_memory(self):
        from mlsl_amd import ops
        counts, n, shard, block = sr.LAYOUTS["edges"], 4, 513, 256
        total = sum(counts)
        vp, _ = wq.shard_input("edges", n, shard, block, "f32")
        want = wq.shard_expectation("edges", n, shard, block, "f32", False)
        flat = torch.from_numpy(np.array(vp[:total], copy=True)).cuda()
        offs = sr.offsets(counts)
        d_offs = torch.from_numpy(offs).cuda()
        d_ptrs = torch.tensor([flat.data_ptr() + 4 * int(o) for o in offs[:-1]],
                              dtype=torch.int64, device="cuda")
        stride = wq.default_stride(shard, block)
        sw = sr.qr.wire_bytes(shard, block)
        wire = torch.full(((n - 1) * stride + sw,), 0xAB, dtype=torch.uint8, device="cuda")
        ops.quantize_gather_shards_tables(d_ptrs, d_offs, len(counts), total, wire, n, shard,
                                          block=block, dtype="f32")
        torch.cuda.synchronize()
        got = wire.cpu().numpy()
        for j in range(n):
            assert np.array_equal(got[j * stride:j * stride + sw], want[j]["wire"]), j

    def test_rejects(self):
        from mlsl_amd import ops
        a = torch.zeros(8, device="cuda")
        b = torch.zeros(8, device="cuda")
        wire = torch.full((2 * sr.qr.wire_bytes(8, 8) + 16,), 0xCD, dtype=torch.uint8,
                          device="cuda")
        f = ops.quantize_gather_shards
        with pytest.raises(ValueError, match="at least one element"):
            f([a, b], [8, 0], wire, 2, 8, block=8)
        with pytest.raises(ValueError, match="at least one segment"):
            f([], [], wire, 2, 8, block=8)
        with pytest.raises(ValueError, match=r"shard \* nshards < total"):
            f([a, b], [8, 8], wire, 2, 7, block=8)
        with pytest.raises(RuntimeError, match="f32/bf16 only"):
            f([a, b], [8, 8], wire, 2, 8, block=8, dtype="f64")
        with pytest.raises(ValueError, match="multiple of 4"):
            f([a, b], [8, 8], wire, 2, 8, block=6)
        with pytest.raises(ValueError, match="wire_stride"):
            f([a, b], [8, 8], wire, 2, 8, block=8, wire_stride=8)
        # the C entry point refuses the same things before it launches
        import ctypes
        L = ops._lib()
        ptrs = (ctypes.c_void_p * 2)(a.data_ptr(), b.data_ptr())
        wp = ctypes.c_void_p(wire.data_ptr())
        for counts, nseg, nshards, shard, stride, block, dt, needle in (
                ([8, 0], 2, 2, 8, 16, 8, 0, "segment 1 is empty"),
                ([8, 8], 0, 2, 8, 16, 8, 0, "at least one"),
                ([8, 8], 2, 2, 7, 16, 8, 0, "shard * nshards < total"),
                ([8, 8], 2, 2, 8, 8, 8, 0, "wire_stride"),
                ([8, 8], 2, 2, 8, 16, 8, 1, "f32/bf16 only"),
                ([8, 8], 2, 2, 8, 16, 6, 0, "multiple of 4")):
            cnt = (ctypes.c_size_t * 2)(*counts)
            assert L.mlsl_hip_quantize_gather_shards(ptrs, cnt, nseg, None, wp, nshards, shard,
                                                     stride, block, dt, 0) != 0
            assert needle in ctypes.string_at(L.mlsl_last_error()).decode()
        torch.cuda.synchronize()
        assert bool((wire == 0xCD).all()) and not a.any() and not b.any(), \
            "a rejected call wrote"


@requires_gpu
class TestCollectiveDevice:
    @pytest.mark.parametrize("algo", ["ring", "direct"])
    @pytest.mark.parametrize("world", [1, 2, 4])
    def test_matches_flat_request(self, world, algo):
        # f32 and bf16, every case of workers_quant_rs_seg.COLL_CASES, three starts
        outs = wq.run_ranks("rs_seg_check", world, device=True, algos=[algo])
        wq.assert_all_checked(outs, world)

    @pytest.mark.parametrize("world", [1, 2, 4])
    def test_block_of_12_matches_flat_request(self, world):
        # a wire block of 20 bytes: the plan's seg_wire is 4 (mod 8)
        outs = wq.run_ranks("rs_seg_check", world, device=True, block=wq.ODD_WIRE_BLOCK)
        wq.assert_all_checked(outs, world)

    def test_without_fused_transfers(self):
        outs = wq.run_ranks("rs_seg_check", 2, device=True,
                            extra_env={"MLSL_P2P_FUSED_MAX_KB": "0"})
        wq.assert_all_checked(outs, 2)

    def test_refusals(self):
        # with a host pointer among the tensors or as recv: named, nothing staged
        wq.run_ranks("rs_seg_refusals", 2, device=True)


@requires_gpu
class TestShardedOptimizerDevice:
    @pytest.mark.parametrize("rs_algo", ["ring", "direct"])
    @pytest.mark.parametrize("world", [2, 4])
    def test_in_place_matches_copy(self, world, rs_algo):
        outs = wq.run_ranks("zero1_check", world, device=True, rs_algo=rs_algo)
        wq.assert_all_checked(outs, world)
