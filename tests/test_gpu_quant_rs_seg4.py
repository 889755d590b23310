"""The int4 reduce-scatter over a list of tensors on one MI355X:
QuantizeGatherShards4Kernel (csrc/hip/kernels.hip) against tests/quant4_ref.py
per shard of the padded concatenation and against the host twin, bit for bit,
on both paths; the request over IPC windows against the flat bits=4 request;
ZeRO-1 with int4 gradients read in place."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import workers_quant_rs_seg4 as w4s  # noqa: E402

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]


class GpuApi:
    def put(self, img):
        return torch.from_numpy(np.array(img, copy=True)).cuda()

    def get(self, buf):
        torch.cuda.synchronize()
        return buf.cpu().numpy()

    def shards4(self, tensors, counts, wire, n, shard, err, block, dtype, stride, path):
        from mlsl_amd import ops
        ops.quantize_gather_shards4(tensors, counts, wire, n, shard, err=err, block=block,
                                    dtype=dtype, wire_stride=stride, path=path)

    def gather4(self, tensors, counts, wire, err, block, dtype):
        from mlsl_amd import ops
        ops.quantize_gather4(tensors, counts, wire, err=err, block=block, dtype=dtype)


# every case on GENERIC; the block-256 ones on FAST and on AUTO (which is FAST)
PATHS = [(name, "generic") for name in w4s.CASES] + \
        [(name, p) for name in ("b256", "b256pad") for p in ("fast", None)]


@pytest.mark.parametrize("misalign", [False, True], ids=["al16", "off1"])
@pytest.mark.parametrize("use_err", [True, False], ids=["err", "noerr"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name,path", PATHS, ids=str)
def test_kernel_against_reference_and_host(name, path, dtype, use_err, misalign):
    torch.cuda.set_device(0)
    gpu = w4s.run_case(GpuApi(), w4s.CASES[name], dtype, use_err, misalign, path)
    host = w4s.run_case(w4s.HostApi(), w4s.CASES[name], dtype, use_err, misalign)
    assert np.array_equal(gpu[0], host[0]) and np.array_equal(gpu[1], host[1])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("path", ["generic", "fast"])
def test_second_trip_starts_in_another_shard(path, dtype):
    from mlsl_amd import ops
    counts, n, shard, block, _ = w4s.TRIPS[path]
    assert -(-shard // block) < ops.quant4_blocks_per_trip(path == "fast") < n * -(-shard // block)
    torch.cuda.set_device(0)
    w4s.run_case(GpuApi(), w4s.TRIPS[path], dtype, True, True, path)


def test_kernel_rejects():
    from mlsl_amd import ops
    a = torch.zeros(8, device="cuda")
    wire = torch.full((64,), 0xCD, dtype=torch.uint8, device="cuda")
    f, args = ops.quantize_gather_shards4, ([a, a], [8, 8], wire, 2)
    with pytest.raises(ValueError, match="multiple of 8 at 4 bits"):
        f(*args, 8, block=12)
    with pytest.raises(RuntimeError, match="f32/bf16 only"):
        f(*args, 8, block=8, dtype="f64")
    with pytest.raises(RuntimeError, match="the fast path needs block 256"):
        f(*args, 8, block=24, path="fast")
    with pytest.raises(ValueError, match="shard \\* nshards < total"):
        f(*args, 7, block=8)
    with pytest.raises(ValueError, match="wire_stride=10"):
        f(*args, 8, block=8, wire_stride=10)
    with pytest.raises(RuntimeError, match="the wire must be 4-byte aligned"):
        f([a, a], [8, 8], wire[2:], 2, 8, block=8)
    # the launcher's own checks, past the wrapper's
    ptrs = torch.zeros(2, dtype=torch.int64, device="cuda")
    offs = torch.tensor([0, 8, 16], dtype=torch.int64, device="cuda")
    for shard, stride, msg in ((7, 16, "shard \\* nshards < total"), (8, 8, "wire_stride is smaller")):
        with pytest.raises(RuntimeError, match=msg):
            ops.check(ops._lib().mlsl_hip_quantize_gather_shards4_tables(
                ptrs.data_ptr(), offs.data_ptr(), 2, None, wire.data_ptr(), 16, 2, shard, stride,
                8, ops.DTYPE["f32"], 0, 0))
    torch.cuda.synchronize()
    assert bool((wire == 0xCD).all()) and not a.any(), "a rejected call wrote"


@pytest.mark.parametrize("world,env", [(1, None), (2, None), (4, None),
                                       (2, {"MLSL_P2P_FUSED_MAX_KB": "0"})], ids=str)
@pytest.mark.parametrize("block", [256, 24])
def test_request_matches_flat_bits4(block, world, env):
    w4s.run_ranks("rs4_check", world, device=True, extra_env=env, block=block)


@pytest.mark.parametrize("world,ag", [(2, "none"), (4, "none"), (2, "int4")])
def test_zero1_int4_in_place(world, ag):
    w4s.run_ranks("zero1_check", world, device=True, ag_compression=ag)
