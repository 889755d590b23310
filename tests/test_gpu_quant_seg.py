"""The quantized allreduce over a list of tensors on one MI355X: the gather
and scatter kernels against the numpy reference, the flat kernels and the
host twins, bit for bit; the request over IPC windows against the flat
quantized request on the materialised concatenation; and
DistributedData(compression="int8") on device tensors.

Kernel paths per layout (csrc/hip/kernels.hip, QuantizeGatherKernel and
DequantizeScatterKernel): a block inside one tensor whose first element there
is 16-byte aligned takes the 4-wide loop, every other block the element walk.
"al16" cases put every tensor on a 16-byte boundary, "off1" cases one element
past one, where no block is aligned and every block walks.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import quant_seg_ref as sr  # noqa: E402
from tests import workers_quant_seg as ws  # noqa: E402

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")


class GpuApi:
    """The kernels on torch uint8 tensors of GPU 0."""

    def put(self, img):
        return torch.from_numpy(np.array(img, copy=True)).cuda()

    def get(self, buf):
        torch.cuda.synchronize()
        return buf.cpu().numpy()

    def quantize_gather(self, tensors, counts, wire, err, block, dtype):
        from mlsl_amd import ops
        ops.quantize_gather(tensors, counts, wire, err=err, block=block, dtype=dtype)

    def dequantize_scatter(self, wire, tensors, counts, block, dtype, post_scale,
                           round_first=False):
        from mlsl_amd import ops
        ops.dequantize_scatter(wire, tensors, counts, block=block, dtype=dtype,
                               post_scale=post_scale, round_first=round_first)

    def quantize(self, inp, wire, count, err, block, dtype):
        from mlsl_amd import ops
        ops.quantize(inp, wire, count, err=err, block=block, dtype=dtype)

    def dequantize(self, wire, out, count, block, dtype):
        from mlsl_amd import ops
        ops.dequantize(wire, out, count, block=block, dtype=dtype)


@requires_gpu
class TestKernels:
    def setup_method(self, _):
        torch.cuda.set_device(0)

    @pytest.mark.parametrize("case", ws.CODEC_PARAMS, ids=ws.codec_id)
    def test_against_numpy_flat_and_host(self, case):
        gpu = ws.run_codec_case(GpuApi(), *case)
        host = ws.run_codec_case(ws.HostApi(), *case)
        assert np.array_equal(gpu["wire"], host["wire"]), "wire differs from the host twin's"
        for key in gpu["outs"]:   # (post_scale, round_first)
            assert np.array_equal(gpu["outs"][key], host["outs"][key]), \
                f"{key}: tensors differ from the host twin's"
        # the residual is defined up to the fusion of v - q*scale (both runs
        # were checked against the two roundings): where the two forms agree,
        # so must the twins
        layout, block, dtype, use_err, _ = case
        if use_err:
            want = sr.gather_expectation(layout, block, dtype, True)
            same = want["err_unfused"].view(gpu["err"].dtype) == \
                want["err_fused"].view(gpu["err"].dtype)
            assert np.array_equal(gpu["err"][same], host["err"][same])

    def test_rejects(self):
        from mlsl_amd import ops
        a = torch.zeros(8, device="cuda")
        b = torch.zeros(8, device="cuda")
        wire = torch.full((sr.qr.wire_bytes(16, 8) + 16,), 0xCD, dtype=torch.uint8,
                          device="cuda")
        with pytest.raises(ValueError, match="at least one element"):
            ops.quantize_gather([a, b], [8, 0], wire, block=8)
        with pytest.raises(ValueError, match="at least one segment"):
            ops.quantize_gather([], [], wire, block=8)
        with pytest.raises(RuntimeError, match="f32/bf16 only"):
            ops.quantize_gather([a, b], [8, 8], wire, block=8, dtype="f64")
        with pytest.raises(ValueError, match="multiple of 4"):
            ops.quantize_gather([a, b], [8, 8], wire, block=6)
        with pytest.raises(ValueError, match="at least one element"):
            ops.dequantize_scatter(wire, [a, b], [0, 8], block=8)
        with pytest.raises(ValueError, match="at least one segment"):
            ops.dequantize_scatter(wire, [], [], block=8)
        with pytest.raises(RuntimeError, match="f32/bf16 only"):
            ops.dequantize_scatter(wire, [a, b], [8, 8], block=8, dtype="f16")
        with pytest.raises(ValueError, match="multiple of 4"):
            ops.dequantize_scatter(wire, [a, b], [8, 8], block=0)
        # the C entry points refuse the same things before they launch
        import ctypes
        L = ops._lib()
        ptrs = (ctypes.c_void_p * 2)(a.data_ptr(), b.data_ptr())
        wp = ctypes.c_void_p(wire.data_ptr())
        for counts, nseg, block, dt, needle in (
                ([8, 0], 2, 8, 0, "segment 1 is empty"), ([8, 8], 0, 8, 0, "at least one"),
                ([8, 8], 2, 8, 1, "f32/bf16 only"), ([8, 8], 2, 6, 0, "multiple of 4")):
            cnt = (ctypes.c_size_t * 2)(*counts)
            assert L.mlsl_hip_quantize_gather(ptrs, cnt, nseg, None, wp, block, dt, 0) != 0
            assert needle in ctypes.string_at(L.mlsl_last_error()).decode()
            assert L.mlsl_hip_dequantize_scatter(wp, ptrs, cnt, nseg, block, dt, 1.0, 0) != 0
            assert needle in ctypes.string_at(L.mlsl_last_error()).decode()
        torch.cuda.synchronize()
        assert bool((wire == 0xCD).all()) and not a.any() and not b.any(), \
            "a rejected call wrote"


@requires_gpu
class TestCollectiveDevice:
    @pytest.mark.parametrize("algo", ["ring", "two_shot"])
    @pytest.mark.parametrize("world", [1, 2, 4])
    def test_matches_flat_request(self, world, algo):
        # f32 and bf16, post_scale 1 and 1/world, both layouts, three starts
        outs = ws.run_ranks("seg_check", world, device=True, algos=[algo])
        ws.assert_ranks_agree(outs, world)

    def test_without_fused_transfers(self):
        outs = ws.run_ranks("seg_check", 2, device=True,
                            extra_env={"MLSL_P2P_FUSED_MAX_KB": "0"})
        ws.assert_ranks_agree(outs, 2)

    def test_refusals(self):
        # with a host pointer in the list: named by its index, nothing staged
        ws.run_ranks("seg_refusals", 2, device=True)


@requires_gpu
class TestDdpDevice:
    @pytest.mark.parametrize("world", [2, 4])
    def test_int8_matches_flat_requests(self, world):
        outs = ws.run_ranks("ddp_check", world, device=True)
        ws.assert_ranks_agree(outs, world)
