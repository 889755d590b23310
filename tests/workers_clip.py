"""Rank workers of ShardedOptimizer(max_grad_norm=) and DistributedData.clip_grad_norm_
(python -m tests.workers_clip <worker> '<json kwargs>') and their runner."""
import json
import math
import os
import subprocess
import sys

import numpy as np

from tests import workers_quant_rs as w
from tests.mp import REPO, free_port

# relative bound of one clipped element against the float64 x * c: half an ulp of
# the stored type, the factor's own f32 rounding, one f32 ulp of slack for sqrt
TOL = {"f32": 2.0 ** -22, "bf16": 2.0 ** -8, "f16": 2.0 ** -10}


def coeff(total, max_norm):
    return min(1.0, float(np.float32(max_norm)) / (math.sqrt(total) + 1e-6))


def run_ranks(worker, world, device=False, **kwargs):
    env = dict(os.environ, WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
               MLSL_PORT=str(free_port()), PYTHONPATH=REPO, QRS_DEVICE=w.qrs_device(device))
    env.pop("MLSL_TRANSPORT", None)
    env.update({"MLSL_TIMEOUT": "90"} if device else {"MLSL_TRANSPORT": "tcp"})
    procs = [subprocess.Popen(
        [sys.executable, "-m", "tests.workers_clip", worker, json.dumps(kwargs)],
        env=dict(env, RANK=str(r)), cwd=REPO, stdout=subprocess.PIPE,
        stderr=subprocess.STDOUT, text=True) for r in range(world)]
    try:
        outs = [p.communicate(timeout=120)[0] for p in procs]
    finally:
        for p in procs:
            p.kill()    # a rank that timed out takes the others down
    failed = [f"--- rank {r} rc={p.returncode} ---\n{o[-3000:]}"
              for r, (p, o) in enumerate(zip(procs, outs)) if p.returncode != 0]
    assert not failed, f"{worker} world={world} failed:\n" + "\n".join(failed)


def zero1_clip(max_norm, compression="none", grads="copy"):
    """One SGD step (lr 1) of ShardedOptimizer(reduce="rs") with and without
    max_grad_norm on identical inputs. The run without it leaves the reduced
    gradient G in own_grad (gathered here), so the reference is p - c * G in
    float64 whatever the wire is; uncompressed, G is the exact mean (multiples of
    1/8). Bound: the clip's 2**-22 of c * G plus SGD's one rounding."""
    mx, bufs, rank, size = w._init()
    import torch
    from mlsl_amd.parallel.zero1 import ShardedOptimizer
    d = mx.Distribution(size, 1)
    dev, sizes, n = "cuda" if bufs.gpu else "cpu", (37, 101, 7), 145   # padded at 2 and 4
    p0 = [np.random.default_rng(5 + k).standard_normal(k).astype(np.float32) for k in sizes]

    def grad(r, j):
        return (np.rint(np.random.default_rng(100 * r + j).standard_normal(sizes[j]) * 24)
                / 8).astype(np.float32)

    def run(**kw):
        params = [torch.nn.Parameter(torch.from_numpy(p.copy()).to(dev)) for p in p0]
        for j in (0, 2):   # parameter 1 has no gradient
            params[j].grad = torch.from_numpy(grad(rank, j)).to(dev)
        opt = ShardedOptimizer(params, torch.optim.SGD, d, reduce="rs", lr=1.0,
                               compression=compression, grads=grads, **kw)
        opt.step()
        return opt

    plain, clipped = run(), run(max_grad_norm=max_norm)
    full = torch.zeros(plain.shard * size, dtype=torch.float32, device=dev)
    if size > 1:
        mx.wait(d.all_gather(plain.own_grad, plain.shard, full, dtype="f32", group="data"))
    else:
        full.copy_(plain.own_grad)
    g = full.cpu().numpy().astype(np.float64)
    assert not g[n:].any(), "padding took part in the gradient"
    if compression == "none":
        mean = np.concatenate([sum(grad(r, j).astype(np.float64) for r in range(size)) / size
                               if j != 1 else np.zeros(sizes[1]) for j in range(3)])
        assert np.array_equal(g[:n], mean)
    total = math.fsum((g * g).tolist())
    c = coeff(total, max_norm)
    got = clipped.flat.cpu().numpy()[:n]
    if c == 1.0:
        assert np.array_equal(got.view(np.uint32), plain.flat.cpu().numpy()[:n].view(np.uint32))
    else:
        want = np.concatenate(p0).astype(np.float64) - c * g[:n]
        err = np.abs(got - want)
        bound = TOL["f32"] * np.abs(c * g[:n]) + 2.0 ** -24 * np.abs(want)
        assert (err <= bound).all(), (size, float((err / np.maximum(bound, 1e-300)).max()))
    norm = float(clipped.grad_norm.cpu())
    assert abs(norm - math.sqrt(total)) <= 1e-12 * math.sqrt(total), (norm, math.sqrt(total))
    d.barrier("global")
    mx.finalize()


def ddp_clip(grads="copy"):
    """DistributedData.clip_grad_norm_ over f32 and bf16 parameters (two dtype
    groups, one total) against float64 numpy. The second backward keeps the old
    gradients alive, so the new ones lie elsewhere and both tables are uploaded
    again; a third call on the same gradients uploads nothing. At world > 1 the
    ranks' clipped gradients are gathered and must be the same bits."""
    mx, bufs, rank, size = w._init()
    import torch
    from mlsl_amd.parallel.ddp import DistributedData
    d = mx.Distribution(size, 1)
    gen = torch.Generator().manual_seed(3)
    shapes = [((33,), torch.float32), ((129,), torch.bfloat16), ((7, 5), torch.float32),
              ((3,), torch.bfloat16)]
    model = torch.nn.ParameterList(
        [torch.nn.Parameter(torch.randn(s, generator=gen).to(dt).cuda()) for s, dt in shapes])
    dd = DistributedData(model, d, grads=grads)
    keep = []
    for it in range(3):
        if it < 2:
            keep.append([p.grad for p in model])
            model.zero_grad(set_to_none=True)
            gen.manual_seed(10 * it + rank)
            sum((p.float() * torch.randn(p.shape, generator=gen).cuda() * 3).sum()
                for p in model).backward()
            dd.finish_gradients()
        before = [p.grad.detach().cpu().double().numpy() for p in model]
        max_norm = 2.0 / (it + 1)   # below the norm the last call left
        norm = dd.clip_grad_norm_(max_norm)
        assert norm.shape == () and norm.dtype == torch.float64 and norm.is_cuda
        total = math.fsum(np.concatenate([(b * b).ravel() for b in before]).tolist())
        c = coeff(total, max_norm)
        assert c < 1.0 and abs(float(norm) - math.sqrt(total)) <= 1e-12 * math.sqrt(total)
        for p, b in zip(model, before):
            err = np.abs(p.grad.cpu().double().numpy() - b * c)
            assert (err <= TOL["f32" if p.dtype == torch.float32 else "bf16"]
                    * np.abs(b * c)).all(), (it, p.shape, float(err.max()))
        assert dd.clip_table_uploads == 2 * min(it + 1, 2), (it, dd.clip_table_uploads)
    if size > 1:
        mine = torch.cat([p.grad.float().reshape(-1) for p in model])
        every = torch.zeros(size * mine.numel(), device="cuda")
        mx.wait(d.all_gather(mine, mine.numel(), every, dtype="f32", group="data"))
        rows = every.cpu().numpy().view(np.uint32).reshape(size, -1)
        assert (rows == rows[0]).all(), "ranks disagree after clip_grad_norm_"
    dd.close()
    d.barrier("global")
    mx.finalize()


if __name__ == "__main__":
    {f.__name__: f for f in (zero1_clip, ddp_clip)}[sys.argv[1]](
        **(json.loads(sys.argv[2]) if len(sys.argv) > 2 else {}))
    print(f"OK {sys.argv[1]} rank={os.environ.get('RANK')}")
