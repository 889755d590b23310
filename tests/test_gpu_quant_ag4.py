"""The int4 accumulating all-gather on one MI355X: DequantizeSegments4's two
kernels (csrc/hip/kernels.hip) bit for bit against numpy and the host twin,
the request with every rank on device 0 over IPC windows, and
ShardedOptimizer(ag_compression="int4"). Cases, reference and workers:
tests/workers_quant_ag4.py; host twin: tests/test_quant_ag4_cpu.py."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import workers_quant_ag4 as wa4  # noqa: E402

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]


@pytest.mark.parametrize("acc", [False, True], ids=["assign", "accumulate"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", wa4.CASES + ["trip-generic", "trip-fast"], ids=str)
def test_kernels_against_reference_and_host(case, dtype, acc):
    torch.cuda.set_device(0)
    if isinstance(case, str):
        paths, case = (case[5:],), wa4.trip_case(case == "trip-fast")
    else:
        fits = case[2] == 256 and case[1] % 256 == case[3] == 0
        paths = (None, "generic", "fast") if fits else (None, "generic")
    host = wa4.run_case(False, case, dtype, acc)
    for path in paths:
        assert np.array_equal(wa4.run_case(True, case, dtype, acc, path), host), path
    if case[3]:
        with pytest.raises(RuntimeError, match="the fast path needs block 256"):
            wa4.run_case(True, case, dtype, acc, "fast")


def test_kernel_rejects():
    from mlsl_amd import ops
    wire = torch.full((72,), 0xCD, dtype=torch.uint8, device="cuda")
    out = torch.full((16,), 7.0, device="cuda")
    with pytest.raises(RuntimeError, match="f32/bf16 only"):
        ops.dequantize_segments4(wire, out.double(), 8, 2, block=8, dtype="f64")
    with pytest.raises(RuntimeError, match="at least one segment"):
        ops.dequantize_segments4(wire, out, 8, 0, block=8)
    with pytest.raises(ValueError, match="multiple of 8 at 4 bits"):
        ops.dequantize_segments4(wire, out, 8, 2, block=12)
    with pytest.raises(RuntimeError, match="wire must be 4-byte aligned"):
        ops.dequantize_segments4(wire[2:], out, 8, 2, block=8)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a rejected call wrote to out"


@pytest.mark.parametrize("world,env", [(1, None), (2, None), (4, None),
                                       (2, {"MLSL_P2P_FUSED_MAX_KB": "0"})], ids=str)
def test_all_gather_bits4(world, env):
    wa4.run_ranks("ag4_check", world, device=True, extra_env=env)


@pytest.mark.parametrize("world,compression,zero_steps", [
    (2, "none", 0), (2, "int4", 0), (4, "none", 0), (4, "int4", 0), (2, "none", 2)])
def test_sharded_optimizer_int4_all_gather(world, compression, zero_steps):
    wa4.run_ranks("zero1_check", world, device=True, compression=compression,
                  zero_steps=zero_steps)
