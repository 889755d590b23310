"""The exact allreduce over a list of tensors on one MI355X: the gather and
scatter kernels (csrc/hip/kernels.hip, ListMoveKernel) against numpy on the
concatenation and against the host twins; the request at n=1 and over IPC
windows against the flat exact all_reduce; DistributedData(grads="in_place")."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import workers_list_exact as wl  # noqa: E402
from tests import workers_quant_seg as ws  # noqa: E402
from tests.test_gpu_quant_seg4 import GpuApi  # noqa: E402  (put / get)

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]


@pytest.mark.parametrize("case", wl.PARAMS, ids=str)
def test_kernels_against_reference_and_host(case):
    torch.cuda.set_device(0)
    gpu = wl.run_list_case(GpuApi(), "", *case)
    host = wl.run_list_case(ws.HostApi(), "host_", *case)
    assert all(np.array_equal(gpu[ps], host[ps]) for ps in host)


@pytest.mark.parametrize("world,env", [(1, None), (1, {"MLSL_USE_GRAPHS": "1"}), (2, None),
                                       (4, None), (2, {"MLSL_P2P_FUSED_MAX_KB": "0"})], ids=str)
def test_request_matches_flat_exact(world, env):
    wl.run_ranks("list_check", world, device=True, extra_env=env)


def test_request_refusals():
    wl.run_ranks("list_refusals", 2, device=True)


@pytest.mark.parametrize("world", [2, 4])
def test_ddp_in_place_matches_flat_requests(world):
    wl.run_ranks("ddp_check", world, device=True, with_f64=True)
