#!/usr/bin/env python3
"""The fused AdamW step (ops.adamw_step), measured on one GPU.

For a shard of --mbytes MiB of gradient in --dtype, in one process and
interleaved round by round:

  ours_fast_a/_b  the kernel with g and out 16-byte aligned, out = the rounded
                  parameter for bf16, none for f32 (what ShardedOptimizer runs);
                  a and b are the same call, their disagreement is the spread
  ours_generic    the same with g and out one element past alignment (the odd shard)
  ours_delta      aligned, out = the delta to a replica (ag_compression)
  torch_fused     torch.optim.AdamW(fused=True) on the shard in the parameter
  torch_foreach   dtype, state in that dtype too: the step ShardedOptimizer takes
                  with a torch class
  torch_passes    torch_fused plus what surrounds it there and the kernel absorbs:
                  own_grad /= world and ops.clip_scale; ours_fast and
                  ours_generic are read against it
  torch_passes_delta  the same plus torch.sub(master, own_param, out=delta), the
                  pass ag_compression adds; ours_delta is read against it
  copy            ops.copy of (12 + element size) bytes per element: as many bytes
                  moved as the aligned kernel with `out` moves (f32 without `out`
                  moves 4 fewer per element; the ratio says so)

The clip coefficient is 1 and world is 1 throughout, so the gradient stays what
it was from call to call; the work does not depend on either. Each call is
timed by a pair of device events; a round is the mean of --iters calls and there
are --rounds interleaved rounds per variant.

One JSON line per configuration. No GPU: exits with an error."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from clip_bench import _measure  # noqa: E402
from ddp_bucket_bench import _stats  # noqa: E402

HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)


def variants(torch, ops, dtype, n):
    """name -> callable, for a shard of n elements."""
    tdt, es = (torch.bfloat16, 2) if dtype == "bf16" else (torch.float32, 4)
    total0 = torch.zeros(1, dtype=torch.float64, device="cuda")   # coefficient 1
    g = (torch.randn(n + 8, dtype=torch.float32, device="cuda") * 0.01).to(tdt)
    low = torch.randn(n + 8, dtype=torch.float32, device="cuda").to(tdt)   # own_param
    delta = torch.zeros(n + 8, dtype=tdt, device="cuda")
    p = low[:n].float()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    step = [0]

    def ours(off, out, replica=None):
        def call():
            step[0] += 1
            ops.adamw_step(g[off:off + n], p, m, v, n, step=step[0], total=total0, max_norm=1.0,
                           out=None if out is None else out[off:off + n],
                           replica=None if replica is None else replica[off:off + n],
                           dtype=dtype, **HP)
        return call

    out = None if dtype == "f32" else low
    res = {"ours_fast_a": ours(0, out), "ours_fast_b": ours(0, out),
           "ours_generic": ours(1, out), "ours_delta": ours(0, delta, low)}

    def torch_opt(**kw):
        par = torch.nn.Parameter(low[:n].clone(), requires_grad=False)
        par.grad = g[:n]
        return par, torch.optim.AdamW([par], **HP, **kw)

    fused, foreach = torch_opt(fused=True), torch_opt(foreach=True)
    res["torch_fused"] = fused[1].step
    res["torch_foreach"] = foreach[1].step

    def passes(with_delta):
        def call():
            gg = g[:n]
            gg /= 1.0
            ops.clip_scale(gg, n, total0, 1.0, dtype=dtype)
            fused[1].step()
            if with_delta:
                torch.sub(fused[0], low[:n], out=delta[:n])
        return call

    res["torch_passes"], res["torch_passes_delta"] = passes(False), passes(True)
    src = torch.empty(n * (12 + es), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    res["copy"] = lambda: ops.copy(dst, src, src.numel())
    return res, (fused, foreach)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbytes", type=int, nargs="+", default=[25, 256])
    ap.add_argument("--dtype", nargs="+", default=["f32", "bf16"])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("adamw_bench measures GPU kernels: no GPU found")
    from mlsl_amd import ops
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    for dtype in args.dtype:
        es = 2 if dtype == "bf16" else 4
        for mb in args.mbytes:
            n = (mb << 20) // es
            fns, keep = variants(torch, ops, dtype, n)
            times = _measure(torch, fns, args)
            del fns, keep
            torch.cuda.empty_cache()
            med = {k: _stats(t)["median"] for k, t in times.items()}
            us = min(med["ours_fast_a"], med["ours_fast_b"])
            moved = n * (24 + (0 if dtype == "f32" else 2 * es))
            print(json.dumps({
                "config": "adamw", "dtype": dtype, "mib": mb, "elements": n,
                "iters": args.iters, "rounds": args.rounds,
                **{f"{k}_us": _stats(t) for k, t in times.items()},
                "ours_spread": round(abs(med["ours_fast_a"] - med["ours_fast_b"]) / us, 4),
                "fast_moved_gbs": round(moved / us / 1e3, 1),
                "fast_over_torch_fused": round(us / med["torch_fused"], 3),
                "fast_over_torch_foreach": round(us / med["torch_foreach"], 3),
                "fast_over_torch_passes": round(us / med["torch_passes"], 3),
                "generic_over_torch_fused": round(med["ours_generic"] / med["torch_fused"], 3),
                "generic_over_torch_passes": round(med["ours_generic"] / med["torch_passes"], 3),
                "delta_over_torch_passes_delta": round(med["ours_delta"] / med["torch_passes_delta"],
                                                      3),
                "fast_over_copy": round(us / med["copy"], 3),
                "generic_over_copy": round(med["ours_generic"] / med["copy"], 3)}), flush=True)


if __name__ == "__main__":
    main()
