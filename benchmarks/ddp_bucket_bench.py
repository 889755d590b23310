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

--bits4 measures the int4 wire instead: gather4 / scatter4 against the flat
quantize4 / dequantize4 (flat_a, flat_b) and, in the same run on the same
tensors, against the int8 list kernels (gather8_*, scatter8_*); --path names
the int4 list kernels' path (fast: one block per half-wave; generic: one wave
per block). In bucket mode both requests run at 4 bits.

--exact measures the exact list request instead. kernels: gather_list and
scatter_scale_list (post_scale 1 and 1/3) against ops.copy of the same bytes
(copy_a, copy_b), on 64 equal tensors at 16-byte aligned bases, on the same 64
each one element past such a base, and on 4096 ragged tensors each at a
16-byte aligned base of its own, as an allocator places them (so the tensor
and flat addresses disagree modulo 16 after the first odd length). bucket: one
SegmentedAllReduce(compression=None) against torch.cat, the flat exact
request, a divide and one copy_ per tensor, on --tensors tensors (64 equal, or
ragged).

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
    bits = 4 if args.bits4 else 8
    wire = torch.empty(ops.wire_bytes(total, block, bits), dtype=torch.uint8, device="cuda")
    if args.bits4:
        quantize, dequantize = ops.quantize4, ops.dequantize4
        gather = lambda *a, **k: ops.quantize_gather4_tables(*a, path=args.path, **k)  # noqa: E731
        scatter = lambda *a, **k: ops.dequantize_scatter4_tables(*a, path=args.path, **k)  # noqa: E731
        wire8 = torch.empty(ops.wire_bytes(total, block), dtype=torch.uint8, device="cuda")
    else:
        quantize, dequantize = ops.quantize, ops.dequantize
        gather, scatter = ops.quantize_gather_tables, ops.dequantize_scatter_tables

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
        variants[f"quantize_{tag}"] = lambda: quantize(src, wire, total, err=err,
                                                       block=block, dtype=args.dtype)
        variants[f"dequantize_{tag}"] = lambda: dequantize(wire, out, total, block=block,
                                                           dtype=args.dtype)
    for name, counts in layouts.items():
        ip, io, n = tables(counts, src)
        op_, oo, _ = tables(counts, out)
        variants[f"gather_{name}"] = (
            lambda ip=ip, io=io, n=n: gather(
                ip, io, n, total, wire, err=err, block=block, dtype=args.dtype))
        variants[f"scatter_{name}"] = (
            lambda op_=op_, oo=oo, n=n: scatter(
                wire, op_, oo, n, total, block=block, dtype=args.dtype, post_scale=0.5))
        if args.bits4:
            # the int8 list kernels on the same tensors, a wire of their own
            variants[f"gather8_{name}"] = (
                lambda ip=ip, io=io, n=n: ops.quantize_gather_tables(
                    ip, io, n, total, wire8, err=err, block=block, dtype=args.dtype))
            variants[f"scatter8_{name}"] = (
                lambda op_=op_, oo=oo, n=n: ops.dequantize_scatter_tables(
                    wire8, op_, oo, n, total, block=block, dtype=args.dtype, post_scale=0.5))

    # same bits before anything is timed (post_scale 1 for the comparison)
    ref_w, ref_o = torch.empty_like(wire), torch.empty_like(out)
    quantize(src, ref_w, total, block=block, dtype=args.dtype)
    dequantize(ref_w, ref_o, total, block=block, dtype=args.dtype)
    for name, counts in layouts.items():
        ip, io, n = tables(counts, src)
        op_, oo, _ = tables(counts, out)
        gather(ip, io, n, total, wire, block=block, dtype=args.dtype)
        scatter(wire, op_, oo, n, total, block=block, dtype=args.dtype)
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

    if args.bits4:
        ops.quantize(src, wire8, total, block=block, dtype=args.dtype)   # for scatter8_*
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
           "block": block, "bits": bits, "path": args.path, "iters": args.iters,
           "rounds": args.rounds, **{f"{k}_us": _stats(v) for k, v in times.items()}}
    for kind, flat in (("gather", "quantize"), ("scatter", "dequantize")):
        a, b = med[f"{flat}_flat_a"], med[f"{flat}_flat_b"]
        res[f"{flat}_flat_spread"] = round(abs(a - b) / min(a, b), 4)
        for name in layouts:
            res[f"{kind}_{name}_over_flat"] = round(med[f"{kind}_{name}"] / min(a, b), 3)
            if args.bits4:
                res[f"{kind}_{name}_over_int8"] = round(
                    med[f"{kind}_{name}"] / med[f"{kind}8_{name}"], 3)
    print(json.dumps(res), flush=True)


def kernels_exact(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("kernels mode measures GPU kernels: no GPU found")
    from mlsl_amd import ops
    torch.cuda.set_device(0)
    es = 2 if args.dtype == "bf16" else 4
    tdt = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    total = (args.mbytes << 20) // es // 4096 * 4096
    torch.manual_seed(0)
    src = (torch.randn(total, dtype=torch.float32, device="cuda") * 0.01).to(tdt)
    flat, back = torch.empty_like(src), torch.empty_like(src)
    g = 16 // es   # elements per 16 bytes

    def place(counts, shift):
        """Tensors of `counts` elements in one arena, every base `shift`
        elements past a 16-byte boundary, holding `src` in order."""
        starts, pos = [], 0
        for n in counts:
            starts.append(pos + shift)
            pos = (pos + shift + n + g - 1) // g * g
        arena = torch.zeros(pos + g, dtype=tdt, device="cuda")
        offs = [0]
        for s, n in zip(starts, counts):
            arena[s:s + n] = src[offs[-1]:offs[-1] + n]
            offs.append(offs[-1] + n)
        ptrs = [arena.data_ptr() + s * es for s in starts]
        return (arena, torch.tensor(ptrs, dtype=torch.int64, device="cuda"),
                torch.tensor(offs, dtype=torch.int64, device="cuda"), len(counts), starts)

    layouts = {"aligned64": place([total // 64] * 64, 0), "off1_64": place([total // 64] * 64, 1),
               "ragged4096": place(_ragged(total, 4096), 0)}
    variants = {f"copy_{t}": (lambda: ops.copy(flat, src, total * es)) for t in ("a", "b")}
    for name, (arena, pp, oo, n, starts) in layouts.items():
        variants[f"gather_{name}"] = lambda pp=pp, oo=oo, n=n: ops.gather_list_tables(
            pp, oo, n, total, flat, dtype=args.dtype)
        for tag, ps in (("scatter1", 1.0), ("scatter3", 1.0 / 3.0)):
            variants[f"{tag}_{name}"] = lambda pp=pp, oo=oo, n=n, ps=ps: \
                ops.scatter_scale_list_tables(flat, pp, oo, n, total, dtype=args.dtype,
                                              post_scale=ps)
        # same bits before anything is timed: there and back again
        flat.zero_()
        ops.gather_list_tables(pp, oo, n, total, flat, dtype=args.dtype)
        assert torch.equal(flat.view(torch.uint8), src.view(torch.uint8)), name
        arena.zero_()
        ops.scatter_scale_list_tables(flat, pp, oo, n, total, dtype=args.dtype)
        ops.gather_list_tables(pp, oo, n, total, back, dtype=args.dtype)
        assert torch.equal(back.view(torch.uint8), src.view(torch.uint8)), name

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
    med = {k: _stats(v)["median"] for k, v in times.items()}
    a, b = med["copy_a"], med["copy_b"]
    res = {"config": "list-exact-kernels", "dtype": args.dtype, "total_mib": total * es >> 20,
           "iters": args.iters, "rounds": args.rounds,
           **{f"{k}_us": _stats(v) for k, v in times.items()},
           "copy_spread": round(abs(a - b) / min(a, b), 4)}
    for k in variants:
        if not k.startswith("copy_"):
            res[f"{k}_over_copy"] = round(med[k] / min(a, b), 3)
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
    nt = args.tensors
    per = (args.mbytes << 20) // es // nt
    # 64 equal tensors, or (--tensors other than 64) ragged ones of the same total
    counts = [per] * nt if nt == 64 else _ragged(per * nt, nt)
    torch.manual_seed(1 + rank)
    grads = [(torch.randn(n, dtype=torch.float32, device="cuda") * 0.01).to(tdt)
             for n in counts]
    d = mx.Distribution(size, 1)
    if args.exact:
        flat_req = mx.PersistentRequest(d, "all_reduce", per * nt, dtype=args.dtype, op="sum",
                                        group="data")
        seg_req = mx.SegmentedAllReduce(d, counts, dtype=args.dtype, group="data",
                                        post_scale=1.0 / size, compression=None)
    else:
        flat_req = mx.PersistentRequest(d, "all_reduce", per * nt, dtype=args.dtype, op="sum",
                                        group="data", quantized=True,
                                        bits=4 if args.bits4 else 8)
        seg_req = mx.SegmentedAllReduce(d, counts, dtype=args.dtype, group="data",
                                        post_scale=1.0 / size,
                                        compression="int4" if args.bits4 else "int8")

    def flat():
        buf = torch.cat([g.reshape(-1) for g in grads])
        flat_req.start(buf, buf)
        flat_req.wait()
        buf /= size
        off = 0
        for g, n in zip(grads, counts):
            g.copy_(buf[off:off + n])
            off += n

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
        res = {"config": "ddp-bucket", "bits": 0 if args.exact else 4 if args.bits4 else 8,
               "dtype": args.dtype,
               "bucket_mib": per * nt * es >> 20,
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
    ap.add_argument("--bits4", action="store_true", help="the int4 wire")
    ap.add_argument("--path", default=None, choices=["fast", "generic"],
                    help="with --bits4 in kernels mode: the int4 list kernels' path")
    ap.add_argument("--exact", action="store_true", help="the exact list request")
    ap.add_argument("--tensors", type=int, default=64,
                    help="bucket mode: tensors in the bucket (64 equal, else ragged)")
    args = ap.parse_args()
    if args.exact and args.bits4:
        ap.error("--exact and --bits4 exclude each other")
    {"kernels": kernels_exact if args.exact else kernels, "bucket": bucket}[args.mode](args)


if __name__ == "__main__":
    main()
