#!/usr/bin/env python3
"""The quantized allreduce over a list of tensors, measured on a GPU.

--mode kernels (one process, n=1): the gather and scatter kernels against the
unchanged flat quantize / dequantize at the same total count, in the same run
and interleaved: --mbytes MiB of --dtype in 64 equal, 16-byte aligned
segments and in 4096 ragged ones (element-aligned, boundaries anywhere). The
segment tables stay in device memory, as a request keeps them. Each call is
timed by a pair of device events on the stream the kernels run on; a round is
the mean of --iters calls and there are --rounds rounds per variant. The flat
kernels run as two variants of their own (flat_a, flat_b): their disagreement
is the run-to-run spread that the margin of a comparison has to exceed.

--mode bucket (benchmarks/mp_run.py --world 2, both ranks on one device): one
DDP bucket of --mbytes MiB in 64 tensors, reduced and averaged in place.
`flat` is what the library offered before: torch.cat, the flat quantized
allreduce, a divide and one copy_ per tensor. `segments` is one
SegmentedAllReduce with post_scale = 1/world. Device events on the compute
stream bracket each whole sequence (the request is waited for before the
closing event is recorded).

One JSON line per configuration. No GPU: exits with an error."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 2), "min": round(v[0], 2), "max": round(v[-1], 2)}


def _ragged(total, nseg):
    """nseg counts >= 1 that sum to total: sizes from 1/8 to 7/4 of the mean,
    and a last one that takes what is left (about 6 % of the total)."""
    mean = total // nseg
    counts = [max(1, mean // 8 + (i * 7919) % (mean * 13 // 8)) for i in range(nseg - 1)]
    rest = total - sum(counts)
    assert rest >= 1, "ragged layout overran the total"
    return counts + [rest]


def kernels(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("kernels mode measures GPU kernels: no GPU found")
    from mlsl_amd import ops
    torch.cuda.set_device(0)
    block = 256
    es = 2 if args.dtype == "bf16" else 4
    tdt = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    total = (args.mbytes << 20) // es // (64 * block) * (64 * block)
    torch.manual_seed(0)
    src = (torch.randn(total, dtype=torch.float32, device="cuda") * 0.01).to(tdt)
    out = torch.empty_like(src)
    err = torch.zeros_like(src)
    wire = torch.empty(ops.wire_bytes(total, block), dtype=torch.uint8, device="cuda")

    def tables(counts, base):
        offs = [0]
        for n in counts:
            offs.append(offs[-1] + n)
        ptrs = [base.data_ptr() + o * es for o in offs[:-1]]
        return (torch.tensor(ptrs, dtype=torch.int64, device="cuda"),
                torch.tensor(offs, dtype=torch.int64, device="cuda"), len(counts))

    layouts = {"aligned64": [total // 64] * 64, "ragged4096": _ragged(total, 4096)}
    variants = {}
    for tag in ("flat_a", "flat_b"):
        variants[f"quantize_{tag}"] = lambda: ops.quantize(src, wire, total, err=err,
                                                           block=block, dtype=args.dtype)
        variants[f"dequantize_{tag}"] = lambda: ops.dequantize(wire, out, total, block=block,
                                                               dtype=args.dtype)
    for name, counts in layouts.items():
        ip, io, n = tables(counts, src)
        op_, oo, _ = tables(counts, out)
        variants[f"gather_{name}"] = (
            lambda ip=ip, io=io, n=n: ops.quantize_gather_tables(
                ip, io, n, total, wire, err=err, block=block, dtype=args.dtype))
        variants[f"scatter_{name}"] = (
            lambda op_=op_, oo=oo, n=n: ops.dequantize_scatter_tables(
                wire, op_, oo, n, total, block=block, dtype=args.dtype, post_scale=0.5))

    # same bits before anything is timed (post_scale 1 for the comparison)
    ref_w, ref_o = torch.empty_like(wire), torch.empty_like(out)
    ops.quantize(src, ref_w, total, block=block, dtype=args.dtype)
    ops.dequantize(ref_w, ref_o, total, block=block, dtype=args.dtype)
    for name, counts in layouts.items():
        ip, io, n = tables(counts, src)
        op_, oo, _ = tables(counts, out)
        ops.quantize_gather_tables(ip, io, n, total, wire, block=block, dtype=args.dtype)
        ops.dequantize_scatter_tables(wire, op_, oo, n, total, block=block, dtype=args.dtype)
        assert torch.equal(wire, ref_w) and torch.equal(out.view(torch.uint8),
                                                        ref_o.view(torch.uint8)), name

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
            err.zero_()
            times[k].append(timed(fn))
    med = {k: _stats(v)["median"] for k, v in times.items()}
    res = {"config": "quant-seg-kernels", "dtype": args.dtype, "total_mib": total * es >> 20,
           "block": block, "iters": args.iters, "rounds": args.rounds,
           **{f"{k}_us": _stats(v) for k, v in times.items()}}
    for kind, flat in (("gather", "quantize"), ("scatter", "dequantize")):
        a, b = med[f"{flat}_flat_a"], med[f"{flat}_flat_b"]
        res[f"{flat}_flat_spread"] = round(abs(a - b) / min(a, b), 4)
        for name in layouts:
            res[f"{kind}_{name}_over_flat"] = round(med[f"{kind}_{name}"] / min(a, b), 3)
    print(json.dumps(res), flush=True)


def bucket(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("bucket mode measures the device transport: no GPU found")
    import mlsl_amd as mx
    mx.init()
    rank, size = mx.rank(), mx.world_size()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)) % torch.cuda.device_count())
    es = 2 if args.dtype == "bf16" else 4
    tdt = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    nt = 64
    per = (args.mbytes << 20) // es // nt
    torch.manual_seed(1 + rank)
    grads = [(torch.randn(per, dtype=torch.float32, device="cuda") * 0.01).to(tdt)
             for _ in range(nt)]
    d = mx.Distribution(size, 1)
    flat_req = mx.PersistentRequest(d, "all_reduce", per * nt, dtype=args.dtype, op="sum",
                                    group="data", quantized=True)
    seg_req = mx.SegmentedAllReduce(d, [per] * nt, dtype=args.dtype, group="data",
                                    post_scale=1.0 / size)

    def flat():
        buf = torch.cat([g.reshape(-1) for g in grads])
        flat_req.start(buf, buf)
        flat_req.wait()
        buf /= size
        off = 0
        for g in grads:
            g.copy_(buf[off:off + per])
            off += per

    def segments():
        seg_req.start(grads)
        seg_req.wait()

    variants = {"flat": flat, "segments": segments}

    def timed(fn):
        ms = 0.0
        for _ in range(args.iters):
            d.barrier("global")
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms += e0.elapsed_time(e1)
        return ms / args.iters

    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn))
    if rank == 0:
        res = {"config": "ddp-bucket", "dtype": args.dtype, "bucket_mib": per * nt * es >> 20,
               "tensors": nt, "world": size, "iters": args.iters, "rounds": args.rounds,
               **{f"{k}_ms": _stats(v) for k, v in times.items()}}
        res["segments_over_flat"] = round(res["segments_ms"]["median"] /
                                          res["flat_ms"]["median"], 3)
        print(json.dumps(res), flush=True)
    flat_req.destroy()
    seg_req.destroy()
    mx.finalize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=["kernels", "bucket"])
    ap.add_argument("--mbytes", type=int, default=25)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    {"kernels": kernels, "bucket": bucket}[args.mode](args)


if __name__ == "__main__":
    main()
