"""The int4 allreduce over a list of tensors: the codec case its CPU and GPU
tests share, and the rank workers (python -m tests.workers_quant_seg4 <worker>
'<json kwargs>'). The reference is tests/quant4_ref.py on the materialised
concatenation; arenas and guards are tests/quant_seg_ref.py's."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

from tests import quant4_ref as q4
from tests import quant_seg_ref as sr
from tests import workers_quant_rs as w
from tests import workers_quant_seg as ws
from tests.mp import REPO, free_port

F32, qr, BITS = np.float32, sr.qr, sr.BITS
# [264, 8, 1008]: five whole 256-blocks, every tensor at a multiple of 8 in V
# (all words vector on aligned bases), the fifth block leaves a half-wave idle
LAYOUTS = {"edges": sr.LAYOUTS["edges"], "tiny700": sr.LAYOUTS["tiny700"],
           "vec1280": [264, 8, 1008], "fastslow": sr.LAYOUTS["fastslow"]}
PARAMS = [(lay, blk, dt, ue, mis, path) for lay in LAYOUTS for blk in (256, 24)
          for dt in ("f32", "bf16") for ue in (False, True) for mis in (False, True)
          for path in ((None, "generic", "fast") if blk == 256 else (None, "generic"))]
# one launch's grid plus three blocks; the second trip starts inside tensor 2
TRIP_PARAMS = [(f"trip-{p}", 256, dt, ue, False, p) for p in ("generic", "fast")
               for dt, ue in (("f32", True), ("bf16", False))]


def counts_of(layout):
    if not layout.startswith("trip-"):
        return LAYOUTS[layout]
    from mlsl_amd import ops
    per_trip = ops.quant4_blocks_per_trip(layout == "trip-fast") * 256
    return [1000, per_trip - 1100, 3 * 256 + 100]


def run_codec_case(api, layout, block, dtype, use_err, misalign, path):
    """api.gather, then api.scatter at post_scale 1 and 1/3 (bf16: both
    roundings), bit for bit against quant4_ref on the concatenation; guards
    around the wire, the residual and every tensor intact, inputs unchanged.
    Returns what was computed, for the comparison of the twins."""
    counts = counts_of(layout)
    count, item = sum(counts), sr.ITEM[dtype]
    nbytes, wbytes = count * item, q4.qr.nblocks(count, block) * (block // 2 + 8)
    v, e0 = q4.make_input(count, block, dtype, seed=count + block)
    want = q4.codec(v, e0 if use_err else None, count, block, dtype)
    arena = sr.Arena(counts, dtype, misalign)
    tensors = lambda buf: [buf[s:s + n * item] for s, n in zip(arena.starts, counts)]  # noqa: E731

    in_img = arena.fill(v)
    d_in = api.put(in_img)
    wire_img, lo = sr.guarded_bytes(wbytes, 0xAB)
    err_img, _ = sr.guarded_bytes(nbytes, e0.view(np.uint8))
    d_wire, d_err = api.put(wire_img), api.put(err_img)
    api.gather(tensors(d_in), counts, d_wire[lo:lo + wbytes],
               d_err[lo:lo + nbytes] if use_err else None, block, dtype, path)
    h_wire, h_err = api.get(d_wire), api.get(d_err)
    wire, err = h_wire[lo:lo + wbytes], h_err[lo:lo + nbytes].view(BITS[dtype])
    assert np.array_equal(api.get(d_in), in_img), "the gather wrote to a tensor"
    assert sr.body_intact(h_wire, wbytes) and sr.body_intact(h_err, nbytes)
    # header word 1, nibbles past count and words past the end are 0 in `want`
    assert np.array_equal(wire, want["wire"]), "wire"
    assert np.array_equal(err, (want["err"] if use_err else e0).view(BITS[dtype])), "residual"

    scales, _, q = q4.unpack(want["wire"], block)
    dq = (q.astype(F32) * scales[:, None]).astype(F32).reshape(-1)[:count]
    outs = {}
    for rf in ((False, True) if dtype == "bf16" else (False,)):
        pre = qr.decode(qr.encode(dq, dtype), dtype) if rf else dq
        for ps in (1.0, 1.0 / 3.0):
            d_out = api.put(arena.blank())
            api.scatter(d_wire[lo:lo + wbytes], tensors(d_out), counts, block, dtype, ps, rf, path)
            h_out = api.get(d_out)
            assert arena.guards_intact(h_out), "write outside the tensors"
            got = arena.gather(h_out).view(BITS[dtype])
            ref = qr.encode((pre * F32(ps)).astype(F32), dtype).view(BITS[dtype])
            assert np.array_equal(got, ref), (ps, rf, int((got != ref).sum()))
            if ps == 1.0:
                assert np.array_equal(got, want["out"].view(BITS[dtype])), "flat dequantize"
            outs[(ps, rf)] = got
    assert np.array_equal(api.get(d_wire), h_wire), "the scatter wrote to the wire"
    return dict(wire=wire.copy(), err=err.copy(), outs=outs)


class HostApi(ws.HostApi):
    def gather(self, tensors, counts, wire, err, block, dtype, path):
        from mlsl_amd import ops
        ops.host_quantize_gather4(tensors, counts, wire, err=err, block=block, dtype=dtype)

    def scatter(self, wire, tensors, counts, block, dtype, ps, rf, path):
        from mlsl_amd import ops
        ops.host_dequantize_scatter4(wire, tensors, counts, block=block, dtype=dtype,
                                     post_scale=ps, round_first=rf)


# ---- ranks -------------------------------------------------------------------

def run_ranks(worker, world, device=False, extra_env=None, **kwargs):
    """ws.run_ranks for this module's workers; MLSL_QUANT_AR_ALGO=ring is set
    and must not be read at 4 bits."""
    port, procs = free_port(), []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MLSL_PORT=str(port), PYTHONPATH=REPO, QRS_DEVICE=w.qrs_device(device),
                   MLSL_QUANT_AR_ALGO="ring", **(extra_env or {}))
        env.pop("MLSL_TRANSPORT", None)
        env.update({"MLSL_TIMEOUT": "90"} if device else {"MLSL_TRANSPORT": "tcp"})
        procs.append(subprocess.Popen(
            [sys.executable, "-m", "tests.workers_quant_seg4", worker, json.dumps(kwargs)],
            env=env, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs, failed = [], []
    for r, p in enumerate(procs):
        try:
            outs.append(p.communicate(timeout=120)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise AssertionError(f"rank {r} timed out ({worker} world={world})")
        if p.returncode != 0:
            failed.append(f"--- rank {r} rc={p.returncode} ---\n{outs[-1][-3000:]}")
    assert not failed, f"{worker} world={world} failed:\n" + "\n".join(failed)
    ws.assert_ranks_agree(outs, world)


def seg4_check():
    """SegmentedAllReduce(compression="int4", post_scale=1/world) against the
    flat bits=4 request on the concatenation times float32(1/world): three
    starts, residual carried, fresh tensors at every start."""
    mx, bufs, rank, size = w._init()
    d = mx.Distribution(size, 1)
    ps = 1.0 / size
    for counts in sr.COLL_LAYOUTS.values():
        count, offs = sum(counts), sr.offsets(counts)
        for dtype in ("f32", "bf16"):
            req = mx.SegmentedAllReduce(d, counts, dtype=dtype, group="data", post_scale=ps,
                                        compression="int4")
            ref = mx.PersistentRequest(d, "all_reduce", count, dtype=dtype, op="sum",
                                       group="data", quantized=True, bits=4)
            keep, h = [], hashlib.sha256()
            for s in range(ws.STARTS):
                x = ws.start_input(rank, s, count, dtype)
                flat = bufs.put(x)
                ref.start(flat, flat)
                ref.wait()
                want = qr.encode((qr.decode(bufs.get(flat, dtype), dtype) * F32(ps))
                                 .astype(F32), dtype).view(BITS[dtype])
                keep.append([bufs.put(x[offs[j]:offs[j + 1]]) for j in range(len(counts))])
                req.start(keep[-1])
                req.wait()
                got = np.concatenate([bufs.get(t, dtype) for t in keep[-1]]).view(BITS[dtype])
                assert np.array_equal(got, want), (size, dtype, count, s, int((got != want).sum()))
                h.update(got.tobytes())
            print(f"DIGEST {rank} {h.hexdigest()}")
            req.destroy()
            ref.destroy()
    d.barrier("global")
    mx.finalize()


def seg4_refusals(plugin=False):
    mx, bufs, rank, size = w._init()
    d = mx.Distribution(size, 1)
    mk = lambda **kw: lambda: mx.SegmentedAllReduce(  # noqa: E731
        d, [8, 8], group="data", **{"compression": "int4", **kw})
    if plugin:
        import ctypes
        from mlsl_amd._lib import lib
        QP = type("QP", (ctypes.Structure,), {"_fields_": [
            (f, ctypes.c_char_p) for f in ("lib_path", "quant", "dequant", "reduce_sum")] + [
            ("block_size", ctypes.c_size_t), ("elem_in_block", ctypes.c_size_t)]})
        env = ctypes.c_void_p()
        assert lib().mlsl_environment_get_env(ctypes.byref(env)) == 0
        assert lib().mlsl_environment_set_quantization_params(
            env, ctypes.byref(QP(w.PLUGIN.encode(), None, None, None, 264, 256))) == 0
        ws._raises(RuntimeError, "4-bit wire codec cannot run with a compression plugin", mk())
        lib().mlsl_environment_set_quantization_params(
            env, ctypes.byref(QP(None, None, None, None, 0, 256)))
    if size > 8:
        ws._raises(RuntimeError, "at most 8 ranks per group (its requantize takes 8 wires); "
                   "use bits=8", mk())
    ws._raises(RuntimeError, "does not run the ring", mk(ar_algo="ring"))
    ws._raises(ValueError, "compression='fp8'", mk(compression="fp8"))
    mx.set_quant_params(12)
    ws._raises(RuntimeError, "multiple of 8 at 4 bits", mk())
    mx.set_quant_params(256)
    print(f"DIGEST {rank} refused")
    d.barrier("global")
    mx.finalize()


def ddp4_check(with_f64=False):
    """DistributedData(compression="int4") against one flat bits=4 request per
    f32 bucket on torch.cat of a twin model's gradients, times float32(1 /
    world); an f64 bucket stays exact. Three iterations, residuals carried."""
    mx, bufs, rank, size = w._init()
    import torch
    from mlsl_amd.parallel import DistributedData
    dev = "cuda" if bufs.gpu else "cpu"
    torch.manual_seed(11)
    model, twin = ws._mlp(torch, with_f64).to(dev), ws._mlp(torch, with_f64).to(dev)
    d = mx.Distribution(size, 1)
    ws._raises(ValueError, "does not run ar_algo='ring'", lambda: DistributedData(
        model, dist=d, compression="int4", ar_algo="ring"))
    dd = DistributedData(model, dist=d, bucket_mb=0.003, compression="int4", ar_algo="two_shot")
    twin.load_state_dict(model.state_dict())
    tw = {id(p): q for p, q in zip(model.parameters(), twin.parameters())}
    refs = [mx.PersistentRequest(d, "all_reduce", sum(p.numel() for p in ps), dtype="f32",
                                 op="sum", group="data", quantized=True, bits=4)
            if seg is not None else None for ps, seg in zip(dd._buckets, dd._seg)]
    assert sum(r is not None for r in refs) == 2 and len(refs) == (3 if with_f64 else 2)
    for it in range(3):
        x = torch.randn(6, 5, generator=torch.Generator().manual_seed(300 + it * size + rank))
        twin.zero_grad(set_to_none=True)
        twin(x.to(dev)).backward()
        model.zero_grad(set_to_none=True)
        model(x.to(dev)).backward()
        dd.finish_gradients()
        if bufs.gpu:
            torch.cuda.synchronize()
        h = hashlib.sha256()
        for ps, ref in zip(dd._buckets, refs):
            flat = torch.cat([tw[id(p)].grad.detach().reshape(-1) for p in ps])
            if ref is None:
                mx.wait(d.all_reduce(flat, flat, flat.numel(), op="sum", dtype="f64",
                                     group="data"))
                if bufs.gpu:
                    torch.cuda.synchronize()
                want = (flat / size).cpu().numpy()
            else:
                ref.start(flat, flat)
                ref.wait()
                if bufs.gpu:
                    torch.cuda.synchronize()
                want = (flat.cpu().numpy() * F32(1.0 / size)).astype(F32)
            got = torch.cat([p.grad.detach().reshape(-1) for p in ps]).cpu().numpy()
            assert np.array_equal(got, want), (it, got.dtype, int((got != want).sum()))
            h.update(got.tobytes())
        print(f"DIGEST {rank} {h.hexdigest()}")
    dd.close()
    for r in refs:
        if r is not None:
            r.destroy()
    d.barrier("global")
    mx.finalize()


if __name__ == "__main__":
    {f.__name__: f for f in (seg4_check, seg4_refusals, ddp4_check)}[sys.argv[1]](
        **(json.loads(sys.argv[2]) if len(sys.argv) > 2 else {}))
    print(f"OK {sys.argv[1]} rank={os.environ.get('RANK')}")
