"""Rank worker of ShardedOptimizer(params, "adamw")
(python -m tests.workers_adamw '<json kwargs>') and its runner."""
import json
import math
import os
import subprocess
import sys

import numpy as np

from tests import adamw_ref as ar
from tests import workers_quant_rs as w
from tests.mp import REPO, free_port


def run_ranks(world, device=False, **kwargs):
    env = dict(os.environ, WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MLSL_TIMEOUT="90",
               MLSL_PORT=str(free_port()), PYTHONPATH=REPO, QRS_DEVICE=w.qrs_device(device))
    env.pop("MLSL_TRANSPORT", None)
    env.update({} if device else {"MLSL_TRANSPORT": "tcp"})
    procs = [subprocess.Popen([sys.executable, "-m", "tests.workers_adamw", json.dumps(kwargs)],
                              env=dict(env, RANK=str(r)), cwd=REPO, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(world)]
    try:
        outs = [p.communicate(timeout=120)[0] for p in procs]
    finally:
        for p in procs:
            p.kill()    # a rank that timed out takes the others down
    assert not any(p.returncode for p in procs), "\n".join(o[-3000:] for o in outs)


def zero1_adamw(dtype="f32", max_norm=None, **kw):
    """Three steps under reduce="rs" against the reference applied to the reduced
    gradient the run left in own_grad (gathered here) and the squared norm it left
    in _norm2. 145 elements: the shard is odd at 1, 2 and 4 ranks, so ranks above
    0 hold views off 16 bytes. Bit for bit: the own shard's master and moments;
    the whole of flat, or under ag_compression flat's equality across ranks."""
    mx, bufs, rank, size = w._init()
    import torch
    from mlsl_amd.parallel.zero1 import ShardedOptimizer
    d = mx.Distribution(size, 1)
    dev, tdt = "cuda" if bufs.gpu else "cpu", {"f32": torch.float32, "bf16": torch.bfloat16}[dtype]
    sizes, hp = (37, 101, 7), dict(ar.HP, lr=1e-2)
    bits = lambda t: (t if dtype == "f32" else t.view(torch.int16)).cpu().numpy().view(  # noqa: E731
        ar.NP_BITS[dtype])
    params = [torch.nn.Parameter(torch.from_numpy(
        np.random.default_rng(5 + k).standard_normal(k).astype(np.float32)).to(tdt).to(dev))
        for k in sizes]
    opt = ShardedOptimizer(params, "adamw", d, reduce="rs", max_grad_norm=max_norm, **hp, **kw)
    shard, own = opt.shard, slice(rank * opt.shard, (rank + 1) * opt.shard)
    p = ar.decode(bits(opt.flat), dtype).copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    for it in range(1, 4):
        sd = opt.state_dict()
        grads = [(np.rint(np.random.default_rng(100 * r + 10 * it + j).standard_normal(sizes[j])
                          * 24) / 8).astype(np.float32) for r in range(size) for j in range(3)]
        for j in (0, 2):   # parameter 1 has no gradient
            params[j].grad = torch.from_numpy(grads[3 * rank + j]).to(tdt).to(dev)
        opt.step()
        full = torch.zeros(shard * size, dtype=tdt, device=dev)
        if size > 1:
            mx.wait(d.all_gather(opt.own_grad, shard, full, dtype=dtype, group="data"))
        else:
            full.copy_(opt.own_grad)
        g = bits(full)
        if dtype == "f32" and not kw:   # the exact sum, not yet averaged
            want = [sum(grads[3 * r + j] for r in range(size)) * (j != 1) for j in range(3)]
            assert np.array_equal(g[:145], np.concatenate(want)) and not g[145:].any()
        scale, total = float(np.float32(1.0 / size)), None
        if max_norm is not None:
            total = float(opt._norm2.cpu())
            exact = math.sqrt(math.fsum((ar.decode(g, dtype).astype(np.float64) ** 2).tolist()))
            assert abs(math.sqrt(total) - exact) <= 1e-12 * exact
            assert abs(float(opt.grad_norm.cpu()) - exact * scale) <= 1e-12 * exact * scale
        p, m, v, out = ar.step(g, p, m, v, dtype, **hp, step=it, grad_scale=scale, total=total,
                               max_norm=max_norm)
        for name, ref in (("master", p), ("exp_avg", m), ("exp_avg_sq", v)):
            got = getattr(opt, name).cpu().numpy()
            assert np.array_equal(got.view(np.uint32), ref[own].view(np.uint32)), (it, name)
        if kw.get("ag_compression", "none") == "none" or size == 1:
            assert np.array_equal(bits(opt.flat), out), (it, "flat")
        else:
            every = torch.zeros(size * size * shard, dtype=tdt, device=dev)
            mx.wait(d.all_gather(opt.flat, size * shard, every, dtype=dtype, group="data"))
            rows = bits(every).reshape(size, -1)
            assert (rows == rows[0]).all(), "replicas differ across ranks"
    if not kw:   # from the checkpoint before it, the third step again: the same bits
        opt.load_state_dict(sd)
        opt.step()
        assert opt.step_count == 3 and np.array_equal(
            opt.master.cpu().numpy().view(np.uint32), p[own].view(np.uint32))
    d.barrier("global")
    mx.finalize()


if __name__ == "__main__":
    zero1_adamw(**json.loads(sys.argv[1]))
