"""The fused AdamW step without a device: the host twin against the numpy
reference, the reference against torch, ShardedOptimizer("adamw") over TCP."""
import numpy as np
import pytest
import torch

from tests import adamw_ref as ar
from tests import workers_adamw as wa


@pytest.mark.parametrize("count", [1, 7, 1025])
@pytest.mark.parametrize("clip", [None, "clips", "coef 1"])
@pytest.mark.parametrize("mode", ar.MODES)
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_host_twin_is_the_reference(dtype, mode, clip, count):
    from mlsl_amd import ops
    g, p, m, v, replica = ar.inputs(count, dtype, seed=count)
    replica = replica if mode == "delta" else None
    total = None if clip is None else float((ar.decode(g, dtype).astype(np.float64) ** 2).sum())
    kw = dict(ar.HP, step=3, grad_scale=0.25, total=total,
              max_norm={None: None, "clips": 1e-3, "coef 1": 1e6}[clip])
    assert clip is None or (ar.coef(total, kw["max_norm"], 0.25) < 1) == (clip == "clips")
    want = ar.step(g, p, m, v, dtype, replica=replica, want_out=mode != "none", **kw)
    out = None if mode == "none" else np.zeros(count, ar.NP_BITS[dtype])
    ops.host_adamw_step(g, p, m, v, count, out=out, replica=replica, dtype=dtype, **kw)
    for name, got, ref in zip("pmv", (p, m, v), want):
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), name
    assert out is None or np.array_equal(out, want[3])


@pytest.mark.parametrize("weight_decay", [0.0, 0.1])
def test_reference_is_adamw(weight_decay):
    hp = dict(ar.HP, weight_decay=weight_decay)
    rng = np.random.default_rng(0)
    p = rng.standard_normal(4096).astype(np.float32)
    m, v = np.zeros_like(p), np.zeros_like(p)
    tp = torch.nn.Parameter(torch.from_numpy(p).double())
    opt = torch.optim.AdamW([tp], **hp)
    for t in range(1, 11):
        g = (rng.standard_normal(4096) * 0.1).astype(np.float32)
        tp.grad = torch.from_numpy(g).double()
        opt.step()
        p, m, v, _ = ar.step(g, p, m, v, "f32", **hp, step=t, want_out=False)
        assert np.abs(p - tp.detach().numpy()).max() <= 1e-5, t


@pytest.mark.parametrize("world", [1, 2])
def test_sharded_optimizer_adamw_tcp(world):
    wa.run_ranks(world, dtype="f32", max_norm=1.0)


A, H = np.ones(8, np.float32), np.ones(8, np.uint16)


@pytest.mark.parametrize("text,kw", [
    ("step count of at least 1", {"step": 0}), ("replica without out", {"replica": A}),
    ("go together", {"total": 1.0}), ("go together", {"max_norm": 1.0}),
    ("float32", {"m": H}), ("supports f32/bf16/f16 only", {"dtype": "f64"}),
    ("16-byte aligned float32", {"m": A[1:], "device": True}), ("only built-in optimizer", None)])
def test_refusals(text, kw):
    from mlsl_amd import ops
    from mlsl_amd.parallel.zero1 import ShardedOptimizer
    with pytest.raises(ValueError, match=text):
        if kw is None:
            ShardedOptimizer([torch.nn.Parameter(torch.zeros(8))], "sgd")
        kw = dict(dict(lr=1e-3, step=1, m=A), **kw)
        (ops.adamw_step if kw.pop("device", False) else ops.host_adamw_step)(
            A, A, kw.pop("m"), A, 4, **kw)
