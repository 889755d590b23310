"""The int4 reduce-scatter over a list of tensors without a GPU: the host twin
of QuantizeGatherShards4 against tests/quant4_ref.py per shard, the request on
TCP against the flat bits=4 request, its refusals, and ZeRO-1 in place."""
import pytest

from tests import workers_quant_rs_seg4 as w4s

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("misalign", [False, True], ids=["al16", "off1"])
@pytest.mark.parametrize("use_err", [True, False], ids=["err", "noerr"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(w4s.CASES) + ["generic"])
def test_host_twin_against_reference(name, dtype, use_err, misalign):
    w4s.run_case(w4s.HostApi(), {**w4s.CASES, **w4s.TRIPS}[name], dtype, use_err, misalign)


def test_host_twin_rejects():
    import numpy as np
    from mlsl_amd import ops
    a, wire = np.zeros(8, np.float32), np.zeros(64, np.uint8)
    f = ops.host_quantize_gather_shards4
    with pytest.raises(ValueError, match="multiple of 8 at 4 bits"):
        f([a, a], [8, 8], wire, 2, 8, block=12)
    with pytest.raises(ValueError, match="shard \\* nshards < total"):
        f([a, a], [8, 8], wire, 2, 7, block=8)
    with pytest.raises(ValueError, match="wire_stride=10"):
        f([a, a], [8, 8], wire, 2, 8, block=8, wire_stride=10)


@pytest.mark.parametrize("block", [256, 24])
@pytest.mark.parametrize("world", [1, 2, 3, 4, 8])
def test_request_matches_flat_bits4_tcp(world, block):
    w4s.run_ranks("rs4_check", world, block=block)


@pytest.mark.parametrize("world,plugin", [(1, True), (9, False)])
def test_refusals(world, plugin):
    if plugin:
        w4s.w.ensure_plugin()
    w4s.run_ranks("rs4_refusals", world, plugin=plugin)


def test_zero1_int4_in_place_tcp():
    w4s.run_ranks("zero1_check", 2)
