#!/usr/bin/env python3
"""The quantized reduce-scatter over a list of tensors, measured on a GPU.

--mode kernels (one process): the prologue alone. `shards` is one
quantize_gather_shards launch over the list (tables resident in device memory,
as a request keeps them); `flat` is ONE flat quantize launch over the whole
materialised buffer: every shard here is whole 256-blocks, so that launch
writes the bytes of the parent commit's prologue, N flat launches of one shard
each, and takes no longer than they do queued back to back (every ops call
ends with a stream synchronise, so N calls would mostly time N of those);
`copy` is the one copy_ per tensor that fills that buffer first (what
ShardedOptimizer(grads="copy") pays before its request starts). All with the
residual. --mbytes MiB of --dtype in 64 equal, 16-byte aligned tensors and in
4096 ragged ones, for N = 2 and 4 shards. Each call is timed by a pair of
device events on the stream the kernels run on; a round is the mean of --iters
calls and there are --rounds interleaved rounds per variant. `flat` runs as
two variants (flat_a, flat_b): their disagreement is the run-to-run spread.
An equal wire against the flat quantize is asserted before anything is timed;
residual elements that differ from it are counted and reported.

--mode request (benchmarks/mp_run.py --world W, every rank on one device): one
gradient set of --mbytes MiB, reduce-scattered. `copy_flat` is the parent
commit's path for the same data: one copy_ per tensor into a flat buffer, then
the flat quantized reduce_scatter into the rank's own slice of it. `segments`
is one SegmentedReduceScatter over the tensors into a shard-sized tensor.
Device events on the compute stream bracket each whole sequence (the request
is waited for before the closing event is recorded), a barrier before each.

One JSON line per configuration. No GPU: exits with an error."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ddp_bucket_bench import _ragged, _stats  # noqa: E402


def _layouts(total):
    return {"aligned64": [total // 64] * 64, "ragged4096": _ragged(total, 4096)}


def _total(mbytes, es):
    # whole 256-blocks per shard at N = 2 and 4, 64 equal tensors
    return (mbytes << 20) // es // (64 * 256) * (64 * 256)


def _offsets(counts):
    offs = [0]
    for n in counts:
        offs.append(offs[-1] + n)
    return offs


def kernels(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("kernels mode measures GPU kernels: no GPU found")
    from mlsl_amd import ops
    torch.cuda.set_device(0)
    block = 256
    es = 2 if args.dtype == "bf16" else 4
    tdt = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    total = _total(args.mbytes, es)
    torch.manual_seed(0)
    src = (torch.randn(total, dtype=torch.float32, device="cuda") * 0.01).to(tdt)
    flat = torch.empty_like(src)
    err = torch.zeros_like(src)

    for nshards in (2, 4):
        shard = total // nshards
        stride = ops.wire_bytes(shard, block)
        wire = torch.empty(nshards * stride, dtype=torch.uint8, device="cuda")

        assert shard % block == 0   # so that one flat launch writes the N shards' bytes

        def flat_quantize(wire=wire):
            ops.quantize(src, wire, total, err=err, block=block, dtype=args.dtype)

        variants = {"flat_a": flat_quantize, "flat_b": flat_quantize}
        err_diff = {}
        for name, counts in _layouts(total).items():
            offs = _offsets(counts)
            d_ptrs = torch.tensor([src.data_ptr() + o * es for o in offs[:-1]],
                                  dtype=torch.int64, device="cuda")
            d_offs = torch.tensor(offs, dtype=torch.int64, device="cuda")
            views = [src[a:b] for a, b in zip(offs[:-1], offs[1:])]

            def shards(d_ptrs=d_ptrs, d_offs=d_offs, n=len(counts), wire=wire, shard=shard,
                       stride=stride, nshards=nshards):
                ops.quantize_gather_shards_tables(d_ptrs, d_offs, n, total, wire, nshards, shard,
                                                  err=err, block=block, dtype=args.dtype,
                                                  wire_stride=stride)

            def copy(views=views, offs=offs):
                for v, a, b in zip(views, offs[:-1], offs[1:]):
                    flat[a:b].copy_(v)

            # same bits before anything is timed
            ref = torch.empty_like(wire)
            err.zero_()
            flat_quantize(wire=ref)
            e_ref = err.clone()
            err.zero_()
            shards()
            torch.cuda.synchronize()
            assert torch.equal(wire, ref), (name, nshards)
            # the residual is defined up to the fusion of v - q*scale: counted
            err_diff[name] = int((err != e_ref).sum())
            variants[f"shards_{name}"] = shards
            variants[f"copy_{name}"] = copy

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
        fl = min(med["flat_a"], med["flat_b"])
        res = {"config": "quant-rs-seg-kernels", "dtype": args.dtype,
               "total_mib": total * es >> 20, "nshards": nshards, "block": block,
               "iters": args.iters, "rounds": args.rounds,
               **{f"{k}_us": _stats(v) for k, v in times.items()},
               "flat_spread": round(abs(med["flat_a"] - med["flat_b"]) / fl, 4),
               "residual_elements_differing_from_flat": err_diff}
        for name in _layouts(total):
            res[f"shards_{name}_over_flat"] = round(med[f"shards_{name}"] / fl, 3)
            res[f"shards_{name}_over_copy_plus_flat"] = round(
                med[f"shards_{name}"] / (fl + med[f"copy_{name}"]), 3)
        print(json.dumps(res), flush=True)


def request(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("request mode measures the device transport: no GPU found")
    import mlsl_amd as mx
    mx.init()
    rank, size = mx.rank(), mx.world_size()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)) % torch.cuda.device_count())
    es = 2 if args.dtype == "bf16" else 4
    tdt = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    total = _total(args.mbytes, es)
    d = mx.Distribution(size, 1)
    shard = (total + size - 1) // size
    torch.manual_seed(1 + rank)
    for name, counts in _layouts(total).items():
        if args.layout not in ("both", name):
            continue
        grads = [(torch.randn(n, dtype=torch.float32, device="cuda") * 0.01).to(tdt)
                 for n in counts]
        offs = _offsets(counts)
        flat_grad = torch.zeros(shard * size, dtype=tdt, device="cuda")
        own = flat_grad[rank * shard:(rank + 1) * shard]
        recv = torch.zeros(shard, dtype=tdt, device="cuda")
        flat_req = mx.PersistentRequest(d, "reduce_scatter", shard, dtype=args.dtype, op="sum",
                                        group="data", quantized=True, algo=args.algo)
        seg_req = mx.SegmentedReduceScatter(d, counts, shard=shard, dtype=args.dtype,
                                            group="data", algo=args.algo)

        def copy_flat():
            for g, a, b in zip(grads, offs[:-1], offs[1:]):
                flat_grad[a:b].copy_(g)
            flat_req.start(flat_grad, own)
            flat_req.wait()

        def segments():
            seg_req.start(grads, recv)
            seg_req.wait()

        variants = {"copy_flat": copy_flat, "segments": segments}

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
        # both requests have seen the same number of starts of the same data;
        # elements that differ between them are counted and reported
        torch.cuda.synchronize()
        differing = int((own != recv).sum())
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                times[k].append(timed(fn))
        if rank == 0:
            res = {"config": "quant-rs-seg-request", "dtype": args.dtype, "layout": name,
                   "total_mib": total * es >> 20, "tensors": len(counts), "world": size,
                   "algo": args.algo or "default", "iters": args.iters, "rounds": args.rounds,
                   "elements_differing_from_copy_flat": differing,
                   **{f"{k}_ms": _stats(v) for k, v in times.items()}}
            res["segments_over_copy_flat"] = round(res["segments_ms"]["median"] /
                                                   res["copy_flat_ms"]["median"], 3)
            print(json.dumps(res), flush=True)
        flat_req.destroy()
        seg_req.destroy()
        del grads, flat_grad, own, recv
    d.barrier("global")
    mx.finalize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=["kernels", "request"])
    ap.add_argument("--mbytes", type=int, default=25)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--layout", default="both", choices=["both", "aligned64", "ragged4096"])
    ap.add_argument("--algo", default=None, choices=["ring", "direct"])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    {"kernels": kernels, "request": request}[args.mode](args)


if __name__ == "__main__":
    main()
