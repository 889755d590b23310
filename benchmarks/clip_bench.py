#!/usr/bin/env python3
"""Gradient clipping's two kernels, measured on one GPU.

flat: ops.sumsq and ops.clip_scale over --mbytes MiB of --dtype against ops.copy
of the same bytes in the same process. `copy` runs as two variants (copy_a,
copy_b): their disagreement is the run-to-run spread the ratios are read
against. sumsq reads what copy reads and writes nothing; clip_scale moves what
copy moves.

list: the pair ops.sumsq_list_tables + ops.clip_scale_list_tables (tables
resident in device memory, as DistributedData keeps them) against
torch.nn.utils.clip_grad_norm_ on the same tensors as gradients, for 64 equal
16-byte aligned tensors and 4096 ragged ones.

Every clip runs with a coefficient of 1 (total 0, or a max_norm far above the
norm), so the data stays what it was from call to call; the kernels and torch's
foreach-mul do the same work whatever the coefficient is. Each call is timed by
a pair of device events on the stream the kernels run on; a round is the mean
of --iters calls and there are --rounds interleaved rounds per variant.

One JSON line per configuration. No GPU: exits with an error."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ddp_bucket_bench import _ragged, _stats  # noqa: E402


def _measure(torch, variants, args):
    def timed(fn):
        us = 0.0
        for _ in range(args.iters):
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            us += e0.elapsed_time(e1) * 1e3
        return us / args.iters

    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbytes", type=int, nargs="+", default=[25, 256])
    ap.add_argument("--dtype", nargs="+", default=["f32", "bf16"])
    ap.add_argument("--list-mbytes", type=int, default=25)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("clip_bench measures GPU kernels: no GPU found")
    from mlsl_amd import ops
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    total0 = torch.zeros(1, dtype=torch.float64, device="cuda")   # coefficient 1
    out = torch.zeros(1, dtype=torch.float64, device="cuda")

    for dtype in args.dtype:
        tdt, es = (torch.bfloat16, 2) if dtype == "bf16" else (torch.float32, 4)
        for mb in args.mbytes:
            n = (mb << 20) // es
            src = (torch.randn(n, dtype=torch.float32, device="cuda") * 0.01).to(tdt)
            dst = torch.empty_like(src)
            copy = lambda: ops.copy(dst, src, n * es)   # noqa: E731
            times = _measure(torch, {
                "copy_a": copy, "copy_b": copy,
                "sumsq": lambda: ops.sumsq(src, n, out, dtype=dtype),
                "clip_scale": lambda: ops.clip_scale(src, n, total0, 1.0, dtype=dtype)}, args)
            med = {k: _stats(v)["median"] for k, v in times.items()}
            cp = min(med["copy_a"], med["copy_b"])
            print(json.dumps({
                "config": "clip-flat", "dtype": dtype, "mib": mb, "iters": args.iters,
                "rounds": args.rounds, **{f"{k}_us": _stats(v) for k, v in times.items()},
                "copy_spread": round(abs(med["copy_a"] - med["copy_b"]) / cp, 4),
                "sumsq_over_copy": round(med["sumsq"] / cp, 3),
                "clip_scale_over_copy": round(med["clip_scale"] / cp, 3),
                "sumsq_read_gbs": round(n * es / med["sumsq"] / 1e3, 1),
                "copy_moved_gbs": round(2 * n * es / cp / 1e3, 1)}), flush=True)

        n = (args.list_mbytes << 20) // es // 64 * 64
        for name, counts in (("aligned64", [n // 64] * 64), ("ragged4096", _ragged(n, 4096))):
            buf = (torch.randn(n, dtype=torch.float32, device="cuda") * 0.01).to(tdt)
            offs = [0]
            for c in counts:
                offs.append(offs[-1] + c)
            params, pbuf = [], torch.zeros_like(buf)
            for a, b in zip(offs[:-1], offs[1:]):
                p = torch.nn.Parameter(pbuf[a:b])
                p.grad = buf[a:b]
                params.append(p)
            d_ptrs = torch.tensor([buf.data_ptr() + o * es for o in offs[:-1]],
                                  dtype=torch.int64, device="cuda")
            d_offs = torch.tensor(offs, dtype=torch.int64, device="cuda")

            def ours():
                ops.sumsq_list_tables(d_ptrs, d_offs, len(counts), n, out, dtype=dtype)
                ops.clip_scale_list_tables(d_ptrs, d_offs, len(counts), n, out, 1e30,
                                           dtype=dtype)

            def theirs():
                torch.nn.utils.clip_grad_norm_(params, 1e30)

            times = _measure(torch, {"ours_a": ours, "ours_b": ours, "torch": theirs}, args)
            med = {k: _stats(v)["median"] for k, v in times.items()}
            us = min(med["ours_a"], med["ours_b"])
            print(json.dumps({
                "config": "clip-list", "dtype": dtype, "mib": args.list_mbytes, "layout": name,
                "nseg": len(counts), "iters": args.iters, "rounds": args.rounds,
                **{f"{k}_us": _stats(v) for k, v in times.items()},
                "ours_spread": round(abs(med["ours_a"] - med["ours_b"]) / us, 4),
                "ours_over_torch": round(us / med["torch"], 3)}), flush=True)


if __name__ == "__main__":
    main()
