"""The int4 allreduce over a list of tensors on one MI355X: QuantizeGather4 and
DequantizeScatter4 (csrc/hip/kernels.hip) against tests/quant4_ref.py on the
concatenation and against the host twins, bit for bit, on both paths; the
request over IPC windows against the flat bits=4 request; int4 DDP."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import workers_quant_seg4 as w4  # noqa: E402

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]


class GpuApi:
    def put(self, img):
        return torch.from_numpy(np.array(img, copy=True)).cuda()

    def get(self, buf):
        torch.cuda.synchronize()
        return buf.cpu().numpy()

    def gather(self, tensors, counts, wire, err, block, dtype, path):
        from mlsl_amd import ops
        ops.quantize_gather4(tensors, counts, wire, err=err, block=block, dtype=dtype, path=path)

    def scatter(self, wire, tensors, counts, block, dtype, ps, rf, path):
        from mlsl_amd import ops
        ops.dequantize_scatter4(wire, tensors, counts, block=block, dtype=dtype, post_scale=ps,
                                round_first=rf, path=path)


@pytest.mark.parametrize("case", w4.PARAMS + w4.TRIP_PARAMS, ids=str)
def test_kernels_against_reference_and_host(case):
    torch.cuda.set_device(0)
    gpu = w4.run_codec_case(GpuApi(), *case)
    host = w4.run_codec_case(w4.HostApi(), *case)
    assert np.array_equal(gpu["wire"], host["wire"]) and np.array_equal(gpu["err"], host["err"])
    assert all(np.array_equal(gpu["outs"][k], host["outs"][k]) for k in host["outs"])


def test_kernel_rejects():
    from mlsl_amd import ops
    a = torch.zeros(8, device="cuda")
    wire = torch.full((64,), 0xCD, dtype=torch.uint8, device="cuda")
    for f, args in ((ops.quantize_gather4, ([a, a], [8, 8], wire)),
                    (ops.dequantize_scatter4, (wire, [a, a], [8, 8]))):
        with pytest.raises(ValueError, match="multiple of 8 at 4 bits"):
            f(*args, block=12)
        with pytest.raises(RuntimeError, match="f32/bf16 only"):
            f(*args, block=8, dtype="f64")
        with pytest.raises(RuntimeError, match="the fast path needs block 256"):
            f(*args, block=24, path="fast")
    with pytest.raises(ValueError, match="at least one segment"):
        ops.quantize_gather4([], [], wire, block=8)
    with pytest.raises(ValueError, match="at least one element"):
        ops.dequantize_scatter4(wire, [a, a], [8, 0], block=8)
    torch.cuda.synchronize()
    assert bool((wire == 0xCD).all()) and not a.any(), "a rejected call wrote"


@pytest.mark.parametrize("world,env", [(1, None), (2, None), (4, None),
                                       (2, {"MLSL_P2P_FUSED_MAX_KB": "0"})], ids=str)
def test_request_matches_flat_bits4(world, env):
    w4.run_ranks("seg4_check", world, device=True, extra_env=env)


@pytest.mark.parametrize("world", [2, 4])
def test_ddp_int4_matches_flat_requests(world):
    w4.run_ranks("ddp4_check", world, device=True)
