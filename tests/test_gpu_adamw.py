"""ops.adamw_step on one device against the numpy reference, bit for bit, and
ShardedOptimizer(params, "adamw") over IPC windows."""
import functools

import numpy as np
import pytest
import torch

from tests import adamw_ref as ar
from tests import workers_adamw as wa

pytestmark = pytest.mark.gpu
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SENT, PAD = 0x5A5A, 8    # PAD elements of SENT each side: 16 bytes and more
KW = dict(ar.HP, step=3, grad_scale=0.25)


def counts():
    """One element; the edges of a state vector (4) and of 16 bytes of a 16-bit
    gradient (8); a wave's tile of 512 and a partial one; a workgroup's four
    tiles plus 1; the grid's second trip with a tile and a tail of 3."""
    from mlsl_amd import ops
    return [1, 3, 4, 5, 7, 8, 9, 777, 2049, ops.adamw_elems_per_trip() + 2048 + 3]


@functools.lru_cache(maxsize=2)
def case(dtype, count):
    """Inputs and the reference's (p, m, v, out) per output mode, computed once."""
    g, p, m, v, replica = ar.inputs(count, dtype, seed=count % 1000)
    want = {mode: ar.step(g, p, m, v, dtype, replica=replica if mode == "delta" else None,
                          want_out=mode != "none", **KW) for mode in ar.MODES}
    return (g, p, m, v, replica), want


def run(dtype, count, mode, off, replica=None, **kw):
    """One launch on fresh buffers, each between PAD sentinels and g, out and
    replica `off` elements past a 16-byte boundary; returns (p, m, v, out) as the
    reference does, having checked the sentinels and that g and replica were only read."""
    from mlsl_amd import ops
    g, p, m, v, rep = case(dtype, count)[0]
    arrays = [g, rep if replica is None else replica, np.zeros(count, g.dtype), p, m, v]
    bufs, views = [], []
    for i, a in enumerate(arrays):
        lo = PAD + (off if i < 3 else 0)
        bufs.append(torch.full((lo + count + PAD,), SENT, device="cuda",
                               dtype=torch.int32 if a.itemsize == 4 else torch.int16))
        views.append(bufs[-1][lo:lo + count])
        views[-1].copy_(torch.from_numpy(a.view(f"i{a.itemsize}")))
    t = [x.view(TORCH_DT[dtype if i < 3 else "f32"]) for i, x in enumerate(views)]
    assert all(x.data_ptr() % 16 == (off * g.itemsize if i < 3 else 0) for i, x in enumerate(t))
    ops.adamw_step(t[0], t[3], t[4], t[5], count, out=None if mode == "none" else t[2],
                   replica=t[1] if mode == "delta" else None, **dict(KW, **kw))
    got = [x.cpu().numpy().view(a.dtype) for x, a in zip(views, arrays)]
    assert same(got[:2], arrays[:2])
    for buf, x in zip(bufs, views):
        x.fill_(SENT)
        assert bool((buf == SENT).all())
    return got[3], got[4], got[5], got[2] if mode != "none" or got[2].any() else None


def same(got, want):
    return all(a is b or np.array_equal(a.view(f"u{a.itemsize}"), b.view(f"u{b.itemsize}"))
               for a, b in zip(got, want))


@pytest.mark.parametrize("off", [0, 1])   # 1: the odd shard, the generic path
@pytest.mark.parametrize("mode", ar.MODES)
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("ci", range(10))   # slowest, so that case() is computed once
def test_step_is_the_reference(dtype, mode, off, ci):
    count = counts()[ci]
    assert same(run(dtype, count, mode, off), case(dtype, count)[1][mode])
    if off == 0 and ci in (6, 7):   # aligned buffers take either path by name
        for path in ("generic", "fast"):
            assert same(run(dtype, count, mode, off, path=path), case(dtype, count)[1][mode])


@pytest.mark.parametrize("dtype,off", [("f32", 1), ("bf16", 0)])
def test_moments_past_the_cache(dtype, off):
    count = (256 << 20) // 12 + 2049    # more than 256 MiB of state: nontemporal m and v
    from mlsl_amd import MlslError
    assert same(run(dtype, count, "param", off), case(dtype, count)[1]["param"])
    with pytest.raises(MlslError, match="fast path needs"):
        run(dtype, 9, "param", 1, path="fast")


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_total_on_the_device(dtype, off):
    count = 777
    (g, p, m, v, _), want = case(dtype, count)
    norm2 = float((ar.decode(g, dtype).astype(np.float64) ** 2).sum())
    for total, max_norm in ((norm2, 1e-3), (norm2, 1e6), (0.0, 1.0)):
        got = run(dtype, count, "param", off, max_norm=max_norm,
                  total=torch.tensor([total], dtype=torch.float64).cuda())
        clips = ar.coef(total, max_norm, KW["grad_scale"]) < 1
        assert clips == (max_norm == 1e-3)
        assert same(got, ar.step(g, p, m, v, dtype, **KW, total=total, max_norm=max_norm))
        assert clips or same(got, want["param"])    # coef 1: the bits without total


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_delta_to_the_rounded_parameter_is_zero(dtype):
    p, _, _, rounded = case(dtype, 777)[1]["param"]    # the replica holds round(new p)
    out = run(dtype, 777, "delta", 0, replica=rounded)[3]
    exact = ar.decode(rounded, dtype) == p
    assert exact.all() or dtype != "f32"
    assert not (out.view(f"u{out.itemsize}")[exact] & ((1 << 8 * out.itemsize - 1) - 1)).any()
    assert np.array_equal(out, ar.encode(p - ar.decode(rounded, dtype), dtype))


@pytest.mark.parametrize("world,dtype,kw", [
    (1, "bf16", {}), (2, "bf16", {}), (4, "bf16", {}), (2, "f32", {}),   # odd shards
    (2, "bf16", {"compression": "int8", "grads": "in_place", "ag_compression": "int8"})])
def test_sharded_optimizer_adamw(world, dtype, kw):
    wa.run_ranks(world, device=True, dtype=dtype, max_norm=1.0, **kw)
