"""The int4 reduce-scatter over a list of tensors: its codec cases and rank
workers (python -m tests.workers_quant_rs_seg4 <worker> '<json kwargs>').

V' is the tensors' concatenation followed by zeros up to n * shard elements;
the reference is tests/quant4_ref.py applied to each shard of V' built in
numpy. A padding element's residual starts as a NaN pattern here: it must
come back untouched, and the wire must be that of zeros.
"""
import json
import os
import subprocess
import sys

import numpy as np

from tests import quant4_ref as q4
from tests import quant_seg_ref as sr
from tests import workers_quant4 as w4
from tests import workers_quant_rs_seg as wrs
from tests.mp import REPO, free_port

w, ws = wrs.w, wrs.ws
ITEM, NP_DT, BITS = sr.ITEM, sr.NP_DT, sr.BITS
TINY70 = [1 + i % 3 for i in range(70)]            # 139 elements
# name: (counts, nshards, shard, block, bytes of stride past one shard's wire)
CASES = {
    # odd shard, partial last word, boundaries inside words, a word of 3 tensors
    "s37": ([5, 1, 3, 20, 40], 2, 37, 8, 12),
    "pad1": ([5, 1, 3, 20, 40], 2, 35, 8, 0),      # total = n * shard - 1
    # a block of 2 real elements then padding; the last shard padding only
    "real2": ([7, 3], 2, 16, 8, 0),
    "tiny70": (TINY70, 3, 47, 8, 0),
    "one": ([5, 1, 3, 20, 40], 1, 69, 8, 0),       # also quantize_gather4's bytes
    "b24": (TINY70, 2, 70, 24, 4),                 # bps 3, stride 4 past the wire
    # block 256, bps 3: the FAST pair (2, 3) spans shards 0 and 1
    "b256": ([300, 1, 255, 513, 700, 200], 3, 700, 256, 0),
    # the same grid, total 1000: block 4 (base 956) is real, its pair's upper
    # block 5 (base 1212) and all after are padding only
    "b256pad": ([300, 1, 255, 444], 3, 700, 256, 0),
    "b512": ([600, 7, 1000, 500], 2, 1100, 512, 0),    # one word per lane
    "b1024": ([600, 7, 1000, 500], 2, 1100, 1024, 0),  # two words per lane
}
# more wire blocks than one trip of the grid (8192 generic, 16384 fast); the
# second trip starts in shard 1
TRIPS = {"generic": ([20001, 30000, 15000], 2, 32797, 8, 0),
         "fast": ([1000001, 2000000, 1198000], 2, 2099197, 256, 0)}


class HostApi(wrs.HostApi):
    def shards4(self, tensors, counts, wire, n, shard, err, block, dtype, stride, path):
        from mlsl_amd import ops
        ops.host_quantize_gather_shards4(tensors, counts, wire, n, shard, err=err, block=block,
                                         dtype=dtype, wire_stride=stride)

    def gather4(self, tensors, counts, wire, err, block, dtype):
        from mlsl_amd import ops
        ops.host_quantize_gather4(tensors, counts, wire, err=err, block=block, dtype=dtype)


def run_case(api, case, dtype, use_err, misalign, path=None):
    """One launch through `api` against quant4_ref per shard, bit for bit:
    wire, residual, inputs unchanged, sentinels around and between."""
    counts, n, shard, block, extra = case
    total, item = sum(counts), ITEM[dtype]
    sw = q4.qr.nblocks(shard, block) * (block // 2 + q4.HDR)
    stride = sw + extra
    rng = np.random.default_rng(total + block)
    vp = np.zeros(n * shard, dtype=np.float32)
    vp[:total] = rng.standard_normal(total) * 3
    ep = np.zeros(n * shard, dtype=np.float32)
    ep[:total] = rng.standard_normal(total) * 0.01
    vp, ep = q4.qr.encode(vp, dtype), q4.qr.encode(ep, dtype)
    err0 = ep.copy().view(BITS[dtype])
    err0[total:] = {"f32": 0x7FC00001, "bf16": 0x7FC1}[dtype]   # NaN: poisons a scale if read
    arena = sr.Arena(counts, dtype, misalign)
    in_img = arena.fill(vp[:total])
    d_in = api.put(in_img)
    tensors = [d_in[s:s + c * item] for s, c in zip(arena.starts, counts)]
    wbytes, ebytes = (n - 1) * stride + sw, n * shard * item
    wire_img, lo = sr.guarded_bytes(wbytes, 0xAB)
    err_img, _ = sr.guarded_bytes(ebytes, err0.view(np.uint8))
    d_wire, d_err = api.put(wire_img), api.put(err_img)
    api.shards4(tensors, counts, d_wire[lo:lo + wbytes], n, shard,
                d_err[lo:lo + ebytes] if use_err else None, block, dtype, stride, path)
    h_wire, h_err, h_in = api.get(d_wire), api.get(d_err), api.get(d_in)
    assert np.array_equal(h_in, in_img), "an input or its arena was written"
    assert sr.body_intact(h_wire, wbytes) and sr.body_intact(h_err, ebytes), \
        "write before or after the wire or the residual"
    wire, err = h_wire[lo:lo + wbytes], h_err[lo:lo + ebytes].view(BITS[dtype])
    want_err = err0.copy()
    for j in range(n):
        sl = slice(j * shard, (j + 1) * shard)
        want = q4.codec(vp[sl], ep[sl] if use_err else None, shard, block, dtype)
        got = wire[j * stride:j * stride + sw]
        assert np.array_equal(got, want["wire"]), (j, np.flatnonzero(got != want["wire"])[:8])
        assert (wire[j * stride + sw:(j + 1) * stride] == 0xAB).all(), f"gap after shard {j}"
        real = slice(j * shard, min((j + 1) * shard, total))
        if use_err and real.stop > real.start:
            want_err[real] = want["err"].view(BITS[dtype])[:real.stop - real.start]
    assert np.array_equal(err, want_err), np.flatnonzero(err != want_err)[:8]
    if n == 1:
        g_wire, g_err = api.put(np.full(sw, 0xAB, np.uint8)), api.put(ep.view(np.uint8))
        api.gather4(tensors, counts, g_wire, g_err if use_err else None, block, dtype)
        assert np.array_equal(api.get(g_wire), wire)
        assert np.array_equal(api.get(g_err).view(BITS[dtype]), err)
    return wire.copy(), err.copy()


def run_ranks(worker, world, device=False, timeout=120, extra_env=None, **kwargs):
    port, procs = free_port(), []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MLSL_PORT=str(port), PYTHONPATH=REPO, QRS_DEVICE=w.qrs_device(device),
                   **w4.ENV, **(extra_env or {}))
        env.pop("MLSL_TRANSPORT", None)
        env.update({"MLSL_TIMEOUT": "90"} if device else {"MLSL_TRANSPORT": "tcp"})
        procs.append(subprocess.Popen(
            [sys.executable, "-m", "tests.workers_quant_rs_seg4", worker, json.dumps(kwargs)],
            env=env, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    failed = []
    for r, p in enumerate(procs):
        try:
            out, _ = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise AssertionError(f"rank {r} timed out ({worker} world={world})")
        if p.returncode != 0:
            failed.append(f"--- rank {r} rc={p.returncode} ---\n{out[-3000:]}")
    assert not failed, f"{worker} world={world} failed:\n" + "\n".join(failed)


def rs4_check(block=256):
    """Three starts of SegmentedReduceScatter(compression="int4"), naming no
    algorithm under MLSL_QUANT_RS_ALGO=ring, against the flat bits=4 request on
    the materialised V': fresh tensors and recv at every start, both residuals
    carried. "five" leaves ranks that own padding only from four ranks on."""
    mx, bufs, rank, size = w._init()
    d = mx.Distribution(size, 1)
    mx.set_quant_params(block)
    keep = []
    for name in ("edges", "five", "edges_wide"):
        counts, shard = wrs.COLL_CASES[name]
        total, offs = sum(counts), sr.offsets(counts)
        shard = None if shard is None else (shard + size - 1) // size
        for dtype in ("f32", "bf16"):
            req = mx.SegmentedReduceScatter(d, counts, shard=shard, dtype=dtype, group="data",
                                            compression="int4")
            ref = mx.PersistentRequest(d, "reduce_scatter", req.shard, dtype=dtype, op="sum",
                                       group="data", quantized=True, bits=4)
            for s in range(wrs.STARTS):
                x = ws.start_input(rank, s, total, dtype)
                vp = np.concatenate([x, np.zeros(size * req.shard - total, dtype=x.dtype)])
                f_recv = bufs.put(np.full(req.shard, 0x4141, dtype=BITS[dtype]).view(NP_DT[dtype]))
                flat = bufs.put(vp)
                ref.start(flat, f_recv)
                ref.wait()
                tensors = [bufs.put(x[offs[j]:offs[j + 1]]) for j in range(len(counts))]
                recv = bufs.put(np.full(req.shard, 0x4242, dtype=BITS[dtype]).view(NP_DT[dtype]))
                keep.append((tensors, recv))
                req.start(tensors, recv)
                req.wait()
                got, want = bufs.get(recv, dtype), bufs.get(f_recv, dtype)
                bad = int((got.view(BITS[dtype]) != want.view(BITS[dtype])).sum())
                assert bad == 0, (size, name, dtype, block, s, f"{bad} of {req.shard} differ")
            req.destroy()
            ref.destroy()
    mx.set_quant_params(256)
    d.barrier("global")
    mx.finalize()


def rs4_refusals(plugin=False):
    """What compression="int4" refuses at creation, by message."""
    mx, bufs, rank, size = w._init()
    d = mx.Distribution(size, 1)
    mk = lambda **kw: lambda: mx.SegmentedReduceScatter(  # noqa: E731
        d, [5, 7], group="data", **kw)
    w4._raises(ValueError, "expected 'int8' or 'int4'", mk(compression="int2"))
    w4._raises(ValueError, "expected 'int8' or 'int4'", mk(compression=None))
    w4._raises(RuntimeError, "does not run the ring", mk(compression="int4", algo="ring"))
    if size > 8:
        w4._raises(RuntimeError, "at most 8 ranks per group (its fan-in takes 8 wires); use "
                   "bits=8", mk(compression="int4"))
    mx.set_quant_params(12)
    w4._raises(RuntimeError, "multiple of 8 at 4 bits", mk(compression="int4"))
    mx.set_quant_params(256)
    if plugin:
        import ctypes
        from mlsl_amd._lib import lib
        fields = ("lib_path", "quant", "dequant", "reduce_sum")
        QP = type("QP", (ctypes.Structure,), {"_fields_": [(f, ctypes.c_char_p) for f in fields] + [
            ("block_size", ctypes.c_size_t), ("elem_in_block", ctypes.c_size_t)]})
        env = ctypes.c_void_p()
        assert lib().mlsl_environment_get_env(ctypes.byref(env)) == 0
        assert lib().mlsl_environment_set_quantization_params(
            env, ctypes.byref(QP(w.PLUGIN.encode(), None, None, None, 264, 256))) == 0
        w4._raises(RuntimeError, "4-bit wire codec cannot run with a compression plugin",
                   mk(compression="int4"))
        lib().mlsl_environment_set_quantization_params(
            env, ctypes.byref(QP(None, None, None, None, 0, 256)))
    d.barrier("global")
    mx.finalize()


def zero1_check(ag_compression="none"):
    """ShardedOptimizer(compression="int4", rs_algo="direct"): grads="in_place"
    against grads="copy" from the same seeds, three steps of SGD with momentum,
    the parameters' bits equal after each. 1245 parameters pad at every world;
    `unused` never gets a gradient; step 1 hands one gradient over
    non-contiguous."""
    mx, bufs, rank, size = w._init()
    import torch
    from mlsl_amd.parallel.zero1 import ShardedOptimizer
    dev = "cuda" if bufs.gpu else "cpu"
    d = mx.Distribution(size, 1)
    models, opts = [], []
    for grads in ("copy", "in_place"):
        torch.manual_seed(11)
        models.append(wrs._net(torch).to(dev))
        opts.append(ShardedOptimizer(models[-1].parameters(), torch.optim.SGD, d, reduce="rs",
                                     compression="int4", rs_algo="direct", grads=grads,
                                     ag_compression=ag_compression, lr=0.05, momentum=0.9))
    copy, inp = opts
    assert copy.shard * size > 1245 and hasattr(copy, "flat_grad")
    assert not hasattr(inp, "flat_grad"), "in_place kept the model-sized gradient buffer"
    assert inp.own_grad.numel() == inp.shard and inp._qrs_seg is not None
    for it in range(3):
        x = torch.randn(6, 5, generator=torch.Generator().manual_seed(300 + it * size + rank))
        for m, o in zip(models, opts):
            o.zero_grad(set_to_none=True)
            m(x.to(dev)).backward()
            assert m.unused.grad is None
            if it == 1:
                m.w2.grad = m.w2.grad.t().contiguous().t()
                assert not m.w2.grad.is_contiguous()
            o.step()
        a = copy.flat.detach().cpu().view(torch.int32).numpy()
        b = inp.flat.detach().cpu().view(torch.int32).numpy()
        assert np.array_equal(a, b), (it, ag_compression, int((a != b).sum()))
        assert a.any()
    d.barrier("global")
    mx.finalize()


if __name__ == "__main__":
    {f.__name__: f for f in (rs4_check, rs4_refusals, zero1_check)}[sys.argv[1]](
        **(json.loads(sys.argv[2]) if len(sys.argv) > 2 else {}))
    print(f"OK {sys.argv[1]} rank={os.environ.get('RANK')}")
