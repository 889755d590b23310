"""ShardedOptimizer(max_grad_norm=) over TCP (the float64 torch fallback); refusals."""
import pytest
import torch

from tests import workers_clip as wc


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("max_norm", [1.0, 1e6])
def test_sharded_optimizer_clips_tcp(world, max_norm):
    wc.run_ranks("zero1_clip", world, max_norm=max_norm)


@pytest.mark.parametrize("bad", [0, -1, float("inf")])
def test_max_grad_norm_refused(bad):
    from mlsl_amd.parallel.zero1 import ShardedOptimizer
    with pytest.raises(ValueError, match="positive finite"):
        ShardedOptimizer([torch.nn.Parameter(torch.zeros(8))], torch.optim.SGD,
                         max_grad_norm=bad)
