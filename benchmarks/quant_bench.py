#!/usr/bin/env python3
"""Driver config 5: int8-quantized allreduce of bf16/f32 gradients
(default 256 MiB) vs the uncompressed path — bandwidth + quantization error.
Launch with torchrun for N>1.

--mode sum_dequant_ab: single-GPU A/B of the quantized reduce-scatter's last
hop — the fused quant_sum_dequant kernel against the sequence it replaces,
quant_accum followed by dequantize of the same wires (--melems elements,
block 256, f32 and bf16; interleaved rounds in one process).
--mode sum_dequant_n_ab: single-GPU A/B of the one-shot reduce-scatter's
fan-in at N = 4 and 8 wires: the fused quant_sum_dequant_n kernel against the
chain of kernels the ring runs on one segment, N-2 quant_accum plus one
quant_sum_dequant (--melems elements, block 256, f32 and bf16).
--mode allreduce (the default): quantized (ring, and two-shot up to 8 ranks)
against exact allreduce of --mbytes MiB, or of --kbytes KiB when given.
--mode sum_requant_n: single-GPU timing of the two-shot allreduce's
quant_sum_requant_n kernel at 2, 4 and 8 wires, out of place and in place,
against its analytic traffic of nwires * (block + 8) bytes read and block + 8
written per unit (--melems Mi elements, block 256).
--mode reduce_scatter: quantized (ring, and direct up to 8 ranks) against
exact reduce-scatter of --melems elements per rank (launch with
benchmarks/mp_run.py for N>1).
--mode dequant_segments_ab: single-GPU A/B of the quantized all-gather's
finish, dequantize_segments at 2, 4 and 8 segments, assigned against
per-segment and flat dequantize calls and accumulated against dequantize into
scratch plus reduce_ (--melems elements in all, block 256, f32 and bf16).
--mode all_gather: quantized all-gather, assign and accumulate, against the
exact all-gather of --melems elements in all (mp_run.py for N>1)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def sum_dequant_ab(args):
    """One line of JSON per dtype. Every op call ends in a stream
    synchronise, so each timing is host clock around `iters` launch+sync
    pairs; `call_overhead_us` is the same loop on one block, i.e. what a
    call costs beyond its kernel (the old sequence pays it twice)."""
    import torch
    if not torch.cuda.is_available():
        sys.exit("sum_dequant_ab measures GPU kernels: no GPU found")
    from mlsl_amd import ops
    torch.cuda.set_device(0)
    count, block = args.melems << 20, 256
    wbytes = ops.wire_bytes(count, block)
    torch.manual_seed(0)
    wires = []
    for mul in (1.0, 7.0):
        v = torch.randn(count, dtype=torch.float32, device="cuda") * mul
        wire = torch.empty(wbytes, dtype=torch.uint8, device="cuda")
        ops.quantize(v, wire, count, block=block, dtype="f32")
        wires.append(wire)
        del v
    a, b = wires
    acc = a.clone()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.iters

    for dtype, tdt, es in (("f32", torch.float32, 4), ("bf16", torch.bfloat16, 2)):
        out = torch.empty(count, dtype=tdt, device="cuda")
        variants = {
            "accum": lambda: ops.quant_accum(acc, b, count, block=block),
            "dequant": lambda: ops.dequantize(acc, out, count, block=block, dtype=dtype),
            "accum_then_dequant": lambda: (
                ops.quant_accum(acc, b, count, block=block),
                ops.dequantize(acc, out, count, block=block, dtype=dtype)),
            "fused": lambda: ops.quant_sum_dequant(a, b, out, count, block=block,
                                                   dtype=dtype),
            "fused_nt": lambda: ops.quant_sum_dequant_nt(a, b, out, count, block=block,
                                                         dtype=dtype),
            "call_overhead": lambda: ops.quant_sum_dequant(a, b, out, block, block=block,
                                                           dtype=dtype),
        }
        for fn in variants.values():       # warm-up: every shape that is timed
            for _ in range(args.warmup):
                fn()
        times = {k: [] for k in variants}
        for _ in range(args.rounds):       # interleaved rounds
            for k, fn in variants.items():
                times[k].append(timed(fn))
        res = {"config": "quant-sum-dequant-ab", "dtype": dtype,
               "melems": args.melems, "block": block, "iters": args.iters,
               "rounds": args.rounds}
        for k, v in times.items():
            res[f"{k}_us_median"] = round(_median(v) * 1e6, 1)
            res[f"{k}_us_min"] = round(min(v) * 1e6, 1)
        # bytes the fused kernel has to move: two payload bytes in (+headers),
        # one element out
        fused_bytes = 2 * wbytes + count * es
        res["fused_TBps"] = round(fused_bytes / _median(times["fused"]) / 1e12, 3)
        res["fused_over_old"] = round(_median(times["fused"]) /
                                      _median(times["accum_then_dequant"]), 3)
        res["fused_nt_over_fused"] = round(_median(times["fused_nt"]) /
                                           _median(times["fused"]), 3)
        print(json.dumps(res), flush=True)
        del out


def sum_dequant_n_ab(args):
    """One line of JSON per (N, dtype). Timing as in sum_dequant_ab: host
    clock around `iters` launch+sync pairs, interleaved rounds. The chain is
    what the ring spends on one segment across its N-1 hops (on N-1 different
    ranks, one after the other); its accumulator is not reset between calls,
    which changes values and not the bytes moved."""
    import torch
    if not torch.cuda.is_available():
        sys.exit("sum_dequant_n_ab measures GPU kernels: no GPU found")
    from mlsl_amd import ops
    torch.cuda.set_device(0)
    count, block = args.melems << 20, 256
    wbytes = ops.wire_bytes(count, block)
    torch.manual_seed(0)
    wires = []
    for k in range(8):
        v = torch.randn(count, dtype=torch.float32, device="cuda") * (1.0 + k)
        wire = torch.empty(wbytes, dtype=torch.uint8, device="cuda")
        ops.quantize(v, wire, count, block=block, dtype="f32")
        wires.append(wire)
        del v
    acc = wires[0].clone()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.iters

    for n in (4, 8):
        for dtype, tdt, es in (("f32", torch.float32, 4), ("bf16", torch.bfloat16, 2)):
            out = torch.empty(count, dtype=tdt, device="cuda")

            def chain():
                for k in range(1, n - 1):
                    ops.quant_accum(acc, wires[k], count, block=block)
                ops.quant_sum_dequant(acc, wires[n - 1], out, count, block=block,
                                      dtype=dtype)

            variants = {
                "chain": chain,
                "fused_n": lambda: ops.quant_sum_dequant_n(wires[:n], out, count,
                                                           block=block, dtype=dtype),
                "call_overhead": lambda: ops.quant_sum_dequant_n(wires[:n], out, block,
                                                                 block=block, dtype=dtype),
            }
            for fn in variants.values():
                for _ in range(args.warmup):
                    fn()
            times = {k: [] for k in variants}
            for _ in range(args.rounds):
                for k, fn in variants.items():
                    times[k].append(timed(fn))
            res = {"config": "quant-sum-dequant-n-ab", "nwires": n, "dtype": dtype,
                   "melems": args.melems, "block": block, "iters": args.iters,
                   "rounds": args.rounds}
            for k, v in times.items():
                res[f"{k}_us_median"] = round(_median(v) * 1e6, 1)
                res[f"{k}_us_min"] = round(min(v) * 1e6, 1)
            # bytes the fused kernel has to move: n wires in, one element out
            fused_bytes = n * wbytes + count * es
            res["fused_n_TBps"] = round(fused_bytes / _median(times["fused_n"]) / 1e12, 3)
            res["fused_n_over_chain"] = round(_median(times["fused_n"]) /
                                              _median(times["chain"]), 3)
            print(json.dumps(res), flush=True)
            del out


def sum_requant_n(args):
    """One line of JSON per wire count. Timing as in sum_dequant_ab: host
    clock around `iters` launch+sync pairs, interleaved rounds;
    `call_overhead` is the same loop on one unit. In place the destination is
    the last wire, as the schedule uses it; it is requantized again and again,
    which changes values and not the bytes moved."""
    import torch
    if not torch.cuda.is_available():
        sys.exit("sum_requant_n measures GPU kernels: no GPU found")
    from mlsl_amd import ops
    torch.cuda.set_device(0)
    count, block = args.melems << 20, 256
    units, wbytes = count // block, ops.wire_bytes(count, block)
    torch.manual_seed(0)
    wires = []
    for k in range(8):
        v = torch.randn(count, dtype=torch.float32, device="cuda") * (1.0 + k)
        wire = torch.empty(wbytes, dtype=torch.uint8, device="cuda")
        ops.quantize(v, wire, count, block=block, dtype="f32")
        wires.append(wire)
        del v
    dst = torch.empty(wbytes, dtype=torch.uint8, device="cuda")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.iters

    for n in (2, 4, 8):
        own = wires[n - 1].clone()
        inplace = wires[:n - 1] + [own]
        variants = {
            "out_of_place": lambda: ops.quant_sum_requant_n(wires[:n], dst, units,
                                                            block=block),
            "in_place": lambda: ops.quant_sum_requant_n(inplace, own, units, block=block),
            "call_overhead": lambda: ops.quant_sum_requant_n(wires[:n], dst, 1, block=block),
        }
        for fn in variants.values():
            for _ in range(args.warmup):
                fn()
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                times[k].append(timed(fn))
        res = {"config": "quant-sum-requant-n", "nwires": n, "melems": args.melems,
               "block": block, "iters": args.iters, "rounds": args.rounds}
        for k, v in times.items():
            res[f"{k}_us_median"] = round(_median(v) * 1e6, 1)
            res[f"{k}_us_min"] = round(min(v) * 1e6, 1)
        traffic = (n + 1) * wbytes   # n wires in, one wire out
        res["traffic_mib"] = traffic >> 20
        res["out_of_place_TBps"] = round(traffic / _median(times["out_of_place"]) / 1e12, 3)
        res["in_place_TBps"] = round(traffic / _median(times["in_place"]) / 1e12, 3)
        print(json.dumps(res), flush=True)
        del own


def dequant_segments_ab(args):
    """One line of JSON per (nseg, dtype): the segmented dequantize of the
    quantized all-gather against what the unchanged kernels offer, --melems
    elements in all. Assign: `segments` against `separate` (nseg dequantize
    calls, one per segment) and `flat` (one dequantize call over the whole
    wire, legal here because segments are whole blocks). Accumulate:
    `segments_acc` against `scratch_reduce` (one flat dequantize into scratch,
    then reduce_ of scratch into out). Timing as in sum_dequant_ab: host clock
    around `iters` launch+sync pairs, interleaved rounds; `separate` pays the
    call overhead nseg times, `scratch_reduce` twice. GB/s against the least
    bytes the kernel must move: the wire in and one element out, plus one
    element in when accumulating."""
    import torch
    if not torch.cuda.is_available():
        sys.exit("dequant_segments_ab measures GPU kernels: no GPU found")
    from mlsl_amd import ops
    torch.cuda.set_device(0)
    total, block = args.melems << 20, 256
    torch.manual_seed(0)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.iters

    for nseg in (2, 4, 8):
        count = total // nseg
        assert count % block == 0
        seg_wire = ops.wire_bytes(count, block)
        wire = torch.empty(nseg * seg_wire, dtype=torch.uint8, device="cuda")
        for j in range(nseg):
            v = torch.randn(count, dtype=torch.float32, device="cuda") * (1.0 + j)
            ops.quantize(v, wire[j * seg_wire:(j + 1) * seg_wire], count, block=block,
                         dtype="f32")
            del v
        for dtype, tdt, es in (("f32", torch.float32, 4), ("bf16", torch.bfloat16, 2)):
            out = torch.zeros(total, dtype=tdt, device="cuda")
            scratch = torch.empty(total, dtype=tdt, device="cuda")

            def separate():
                for j in range(nseg):
                    ops.dequantize(wire[j * seg_wire:(j + 1) * seg_wire],
                                   out[j * count:(j + 1) * count], count, block=block,
                                   dtype=dtype)

            variants = {
                "segments": lambda: ops.dequantize_segments(wire, out, count, nseg,
                                                            block=block, dtype=dtype),
                "separate": separate,
                "flat": lambda: ops.dequantize(wire, out, total, block=block, dtype=dtype),
                "segments_acc": lambda: ops.dequantize_segments(
                    wire, out, count, nseg, block=block, dtype=dtype, accumulate=True),
                "scratch_reduce": lambda: (
                    ops.dequantize(wire, scratch, total, block=block, dtype=dtype),
                    ops.reduce_(out, scratch, total, dtype=dtype, op="sum")),
                "call_overhead": lambda: ops.dequantize_segments(wire, out, block, 1,
                                                                 block=block, dtype=dtype),
            }
            # same bits before anything is timed
            ref = torch.empty_like(out)
            ops.dequantize(wire, ref, total, block=block, dtype=dtype)
            variants["segments"]()
            assert torch.equal(out.view(torch.uint8), ref.view(torch.uint8))
            for fn in variants.values():
                for _ in range(args.warmup):
                    fn()
            times = {k: [] for k in variants}
            for _ in range(args.rounds):
                for k, fn in variants.items():
                    out.zero_()    # accumulating variants must not run off to inf
                    times[k].append(timed(fn))
            res = {"config": "dequant-segments-ab", "nseg": nseg, "dtype": dtype,
                   "melems": args.melems, "block": block, "iters": args.iters,
                   "rounds": args.rounds}
            for k, v in times.items():
                res[f"{k}_us_median"] = round(_median(v) * 1e6, 1)
                res[f"{k}_us_min"] = round(min(v) * 1e6, 1)
            wbytes = nseg * seg_wire
            res["assign_min_bytes_per_elem"] = round((wbytes + total * es) / total, 3)
            res["acc_min_bytes_per_elem"] = round((wbytes + 2 * total * es) / total, 3)
            res["segments_GBps"] = round((wbytes + total * es) /
                                         _median(times["segments"]) / 1e9, 1)
            res["flat_GBps"] = round((wbytes + total * es) / _median(times["flat"]) / 1e9, 1)
            res["segments_acc_GBps"] = round((wbytes + 2 * total * es) /
                                             _median(times["segments_acc"]) / 1e9, 1)
            res["segments_over_separate"] = round(_median(times["segments"]) /
                                                  _median(times["separate"]), 3)
            res["segments_over_flat"] = round(_median(times["segments"]) /
                                              _median(times["flat"]), 3)
            res["acc_over_scratch_reduce"] = round(_median(times["segments_acc"]) /
                                                   _median(times["scratch_reduce"]), 3)
            print(json.dumps(res), flush=True)
            del out, scratch, ref
        del wire


def all_gather_bench(args):
    """Quantized all-gather, assign and accumulate, against the exact
    all-gather of the same elements: --melems elements in all, 1/world of
    them from each rank (launch with benchmarks/mp_run.py for N>1).
    --exact-only times the exact request alone."""
    import torch
    if not torch.cuda.is_available():
        sys.exit("all_gather mode measures the device transport: no GPU found")
    import mlsl_amd as mx
    mx.init()
    rank, size = mx.rank(), mx.world_size()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)) % torch.cuda.device_count())
    es = 2 if args.dtype == "bf16" else 4
    tdt = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    count = (args.melems << 20) // size // 256 * 256
    torch.manual_seed(1 + rank)
    send = (torch.randn(count, dtype=torch.float32, device="cuda") * 0.01).to(tdt)
    d = mx.Distribution(size, 1)
    reqs = [("exact", mx.PersistentRequest(d, "all_gather", count, dtype=args.dtype,
                                           group="data"))]
    if not args.exact_only:
        reqs += [("int8_assign", mx.PersistentRequest(
                      d, "all_gather", count, dtype=args.dtype, group="data",
                      quantized=True)),
                 ("int8_accumulate", mx.PersistentRequest(
                      d, "all_gather", count, dtype=args.dtype, group="data",
                      quantized=True, accumulate=True))]
    results, outs = {}, {}
    for name, req in reqs:
        recv = torch.zeros(size * count, dtype=tdt, device="cuda")

        def run():
            req.start(send, recv)
            req.wait()

        for _ in range(args.warmup):
            run()
        recv.zero_()
        torch.cuda.synchronize()
        d.barrier("global")
        t0 = time.perf_counter()
        for _ in range(args.iters):
            run()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.iters
        results[name] = {"ms": round(dt * 1e3, 3),
                         "algbw_GBps": round(size * count * es / dt / 1e9, 2)}
        outs[name] = recv
    res = {"config": "int8-quantized-all-gather", "dtype": args.dtype,
           "total_mib": size * count * es >> 20, "world": size,
           **{f"{k}_{kk}": vv for k, v in results.items() for kk, vv in v.items()}}
    if not args.exact_only:
        x = outs["exact"].float()
        res["assign_max_abs_err"] = round((outs["int8_assign"].float() - x).abs().max().item(), 8)
        res["half_step"] = round(x.abs().max().item() / 254.0, 8)
    if rank == 0:
        print(json.dumps(res), flush=True)
    for _, req in reqs:
        req.destroy()
    mx.finalize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="allreduce",
                    choices=["allreduce", "reduce_scatter", "all_gather", "sum_dequant_ab",
                             "sum_dequant_n_ab", "dequant_segments_ab", "sum_requant_n"])
    ap.add_argument("--exact-only", action="store_true",
                    help="all_gather mode: time the exact request alone")
    ap.add_argument("--melems", type=int, default=64,
                    help="Mi elements (per rank) for the reduce-scatter and kernel A/B modes")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mbytes", type=int, default=256)
    ap.add_argument("--kbytes", type=int, default=0,
                    help="allreduce mode: message size in KiB instead of --mbytes")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--device", default="auto")
    args = ap.parse_args()
    if args.mode == "sum_dequant_ab":
        return sum_dequant_ab(args)
    if args.mode == "sum_dequant_n_ab":
        return sum_dequant_n_ab(args)
    if args.mode == "dequant_segments_ab":
        return dequant_segments_ab(args)
    if args.mode == "sum_requant_n":
        return sum_requant_n(args)
    if args.mode == "all_gather":
        return all_gather_bench(args)
    rs = args.mode == "reduce_scatter"

    use_cuda = False
    torch = None
    if args.device in ("auto", "cuda"):
        try:
            import torch as _t
            torch = _t
            use_cuda = torch.cuda.is_available()
        except ImportError:
            pass
    if not use_cuda:
        os.environ.setdefault("MLSL_TRANSPORT", "tcp")

    import mlsl_amd as mx
    mx.init()
    rank, size = mx.rank(), mx.world_size()
    es = 2 if args.dtype == "bf16" else 4
    nbytes = args.kbytes * 1024 if args.kbytes else args.mbytes * 1024 * 1024
    count = nbytes // es
    if rs:
        # `count` stays the send buffer's length; every rank receives 1/size
        count = (args.melems << 20) // size * size

    if use_cuda:
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)) %
                              torch.cuda.device_count())
        tdt = torch.bfloat16 if args.dtype == "bf16" else torch.float32
        g = (torch.randn(count, dtype=torch.float32, device="cuda") * 0.01).to(tdt)
        out_q = torch.empty_like(g)
        out_x = torch.empty_like(g)
    else:
        import numpy as np
        if args.dtype == "bf16":
            print("bf16 on CPU host path unsupported; use --dtype f32",
                  file=sys.stderr)
            args.dtype = "f32"
            es = 4
            count = nbytes // es
        g = (np.random.randn(count) * 0.01).astype(np.float32)
        out_q = np.empty_like(g)
        out_x = np.empty_like(g)

    d = mx.Distribution(size, 1)
    kind, req_count = ("reduce_scatter", count // size) if rs else ("all_reduce", count)
    qreq = mx.PersistentRequest(d, kind, req_count, dtype=args.dtype,
                                op="sum", group="data", quantized=True)
    xreq = mx.PersistentRequest(d, kind, req_count, dtype=args.dtype,
                                op="sum", group="data")
    # the one-shot quantized reduce-scatter, or the two-shot quantized
    # allreduce, next to the ring (the default)
    dreq = None
    if rs and size <= 8:
        dreq = mx.PersistentRequest(d, kind, req_count, dtype=args.dtype, op="sum",
                                    group="data", quantized=True, algo="direct")
    elif size <= 8:
        dreq = mx.PersistentRequest(d, kind, req_count, dtype=args.dtype, op="sum",
                                    group="data", quantized=True, ar_algo="two_shot")
    if rs:
        out_q, out_x = out_q[:req_count], out_x[:req_count]

    def sync():
        if use_cuda:
            torch.cuda.synchronize()

    def run(req, out):
        req.start(g, out)
        req.wait()

    results = {}
    todo = [("quantized", qreq, out_q), ("exact", xreq, out_x)]
    if dreq is not None:
        out_d = out_q.clone() if use_cuda else out_q.copy()
        todo.insert(1, ("quantized_direct" if rs else "quantized_two_shot", dreq, out_d))
    for name, req, out in todo:
        for _ in range(args.warmup):
            run(req, out)
        sync()
        d.barrier("global")
        t0 = time.perf_counter()
        for _ in range(args.iters):
            run(req, out)
        sync()
        dt = (time.perf_counter() - t0) / args.iters
        results[name] = {"ms": round(dt * 1e3, 3),
                         "algbw_GBps": round(count * es / dt / 1e9, 2)}

    # error of the quantized result vs the exact sum
    extra = {}
    if use_cuda:
        err = (out_q.float() - out_x.float()).abs().max().item()
        step = out_x.float().abs().max().item() / 127.0
        if dreq is not None and not rs:
            extra["two_shot_max_abs_err"] = round(
                (out_d.float() - out_x.float()).abs().max().item(), 6)
    else:
        import numpy as np
        err = float(np.abs(out_q - out_x).max())
        step = float(np.abs(out_x).max()) / 127.0
        if dreq is not None and not rs:
            extra["two_shot_max_abs_err"] = round(float(np.abs(out_d - out_x).max()), 6)

    if rank == 0:
        print(json.dumps({
            "config": "int8-quantized-reduce-scatter" if rs
                      else "int8-quantized-allreduce",
            "dtype": args.dtype,
            "message_mib": count * es >> 20,
            "message_bytes": count * es,
            "world": size,
            **{f"{k}_{kk}": vv for k, v in results.items() for kk, vv in v.items()},
            "wire_compression": round(es / ((256 + 8) / 256), 2),
            "max_abs_err": round(err, 6),
            "per_block_step": round(step, 6),
            **extra,
        }))
    qreq.destroy()
    xreq.destroy()
    if dreq is not None:
        dreq.destroy()
    mx.finalize()


if __name__ == "__main__":
    main()
