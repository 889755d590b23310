"""The int4 accumulating all-gather on the host: HostDequantizeSegments at 4
bits against numpy, the request over TCP, ShardedOptimizer(ag_compression=
"int4"). The GPU twin is tests/test_gpu_quant_ag4.py."""
import pytest

from tests import workers_quant_ag4 as wa4
from tests import workers_quant_rs as w


@pytest.mark.parametrize("acc", [False, True], ids=["assign", "accumulate"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", wa4.CASES + ["trip-generic"], ids=str)
def test_host_twin_against_reference(case, dtype, acc):
    wa4.run_case(False, wa4.trip_case(False) if case == "trip-generic" else case, dtype, acc)


@pytest.mark.parametrize("world", [1, 2, 3, 4, 9])
def test_all_gather_bits4(world):
    wa4.run_ranks("ag4_check", world)


def test_all_gather_bits4_refusals():
    w.ensure_plugin()
    wa4.run_ranks("refusals", 1)


@pytest.mark.parametrize("compression,zero_steps", [("none", 0), ("int4", 0), ("none", 2)])
def test_sharded_optimizer_int4_all_gather(compression, zero_steps):
    wa4.run_ranks("zero1_check", 2, compression=compression, zero_steps=zero_steps)
