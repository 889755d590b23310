"""The exact allreduce over a list of tensors on the CPU: the host twins of the
gather and scatter kernels against numpy on the concatenation;
SegmentedAllReduce(compression=None) over TCP against the flat exact
all_reduce; its refusals; DistributedData(grads="in_place")."""
import pytest

torch = pytest.importorskip("torch")

from tests import workers_list_exact as wl  # noqa: E402
from tests import workers_quant_seg as ws  # noqa: E402


@pytest.mark.parametrize("case", wl.PARAMS, ids=str)
def test_host_twins(case):
    wl.run_list_case(ws.HostApi(), "host_", *case)


@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_request_matches_flat_exact(world):
    wl.run_ranks("list_check", world)


def test_request_refusals():
    wl.run_ranks("list_refusals", 2)


@pytest.mark.parametrize("with_f64", [False, True])
def test_ddp_in_place_matches_flat_requests(with_f64):
    wl.run_ranks("ddp_check", 2, with_f64=with_f64)
