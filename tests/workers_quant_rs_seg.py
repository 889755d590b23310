"""The quantized reduce-scatter over a list of tensors: what its tests share,
and their rank workers.

V' is the concatenation of the tensors followed by zeros up to N * shard
elements; it is never built by the code under test, and is built here for the
reference. Codec cases run through `run_shard_case` with an `api` object that
says where the bytes live (numpy for the host twin, torch on GPU 0 for the
kernel). Collective workers compare every start of a `SegmentedReduceScatter`
with the existing flat quantized `PersistentRequest("reduce_scatter")` on the
materialised V': same wire, same residual, so `recv` must agree bit for bit on
every rank. Transport: TCP with numpy buffers, or every rank on GPU 0 with
torch buffers (QRS_DEVICE picks, as in workers_quant_rs).

The residual of a padding element is +0 when a request is created and nothing
ever changes it, so the codec cases start it at +0 there too; on the tensors'
elements it starts non-zero.

Run as: python -m tests.workers_quant_rs_seg <worker> '<json kwargs>'
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np

from tests import quant_ref as qr
from tests import quant_seg_ref as sr
from tests import workers_quant_rs as w
from tests import workers_quant_seg as ws
from tests.mp import REPO, free_port

F32 = np.float32
ITEM, NP_DT, BITS = sr.ITEM, sr.NP_DT, sr.BITS

# (layout, N, shard): the smallest shapes at which each hazard appears
SHARD_CASES = [
    # no padding; shard 1 starts at an odd element: misaligned in the residual
    # and in the tensors, so the register path gives way per block
    ("fastslow", 2, 907),
    # exact fit, both shard boundaries inside tensors
    ("edges", 3, 428),
    # boundaries on a tensor boundary (257) and one past one; one padding element
    ("edges", 5, 257),
    # boundary on a tensor boundary; shard 1 ends with 2 real + 254 padding
    # elements, then a partial block of padding only
    ("edges", 2, 770),
    # shard 2 partly padding, shard 3 all padding (two blocks and one element)
    ("edges", 4, 513),
    # one padding element, many table entries per block
    ("tiny700", 8, 175),
    # one shard: also quantize_gather's bytes
    ("one", 1, 1000),
]
# 8596 wire blocks: a second trip round the grid that starts inside a tensor
# and crosses the shard boundary
BIG_CASE = ("big", 2, 1100033)

SHARD_PARAMS = [(layout, n, shard, block, dtype, use_err, misalign)
                for layout, n, shard in SHARD_CASES for block in sr.BLOCKS
                for dtype in ("f32", "bf16") for use_err in (True, False)
                for misalign in (False, True)] + \
               [BIG_CASE + (256, dtype, True, False) for dtype in ("f32", "bf16")]


def shard_id(p):
    layout, n, shard, block, dtype, use_err, misalign = p
    return f"{layout}-n{n}-s{shard}-{block}-{dtype}-{'err' if use_err else 'noerr'}-" \
           f"{'off1' if misalign else 'al16'}"


def default_stride(shard, block):
    return (qr.wire_bytes(shard, block) + 15) // 16 * 16


class HostApi(ws.HostApi):
    def quantize_gather_shards(self, tensors, counts, wire, nshards, shard, err, block, dtype,
                               wire_stride):
        from mlsl_amd import ops
        ops.host_quantize_gather_shards(tensors, counts, wire, nshards, shard, err=err,
                                        block=block, dtype=dtype, wire_stride=wire_stride)


@functools.lru_cache(maxsize=None)
def shard_input(layout, n, shard, block, dtype):
    """(V', err0') of a case in `dtype` storage, read-only: the layout's
    concatenation and residual (quant_seg_ref.case_input), each followed by
    zeros up to n * shard elements."""
    v, e = sr.case_input(layout, block, dtype)
    pad = np.zeros(n * shard - v.size, dtype=v.dtype)
    vp, ep = np.concatenate([v, pad]), np.concatenate([e, pad])
    vp.setflags(write=False)
    ep.setflags(write=False)
    return vp, ep


@functools.lru_cache(maxsize=None)
def shard_expectation(layout, n, shard, block, dtype, use_err):
    """qr.codec_expectation of every shard of V', read-only."""
    vp, ep = shard_input(layout, n, shard, block, dtype)
    out = []
    for j in range(n):
        sl = slice(j * shard, (j + 1) * shard)
        want = qr.codec_expectation(vp[sl], ep[sl] if use_err else None, shard, block, dtype)
        for a in want.values():
            a.setflags(write=False)
        out.append(want)
    return out


def run_shard_case(api, layout, n, shard, block, dtype, use_err, misalign, wire_stride=None):
    """quantize_gather_shards of one case through `api`, against the numpy
    reference of every shard of V' and against the flat quantize of the same
    `api` launched per shard on the materialised V'. Bit for bit; the residual
    has to be one of the two roundings quant_ref allows and equal to the flat
    quantize's. Sentinels around the wire, the residual and every tensor must
    survive, and so must the bytes between two shards' wires.
    Returns dict(wire, err)."""
    counts = sr.LAYOUTS[layout]
    total, item = sum(counts), ITEM[dtype]
    assert n * shard >= total
    stride = default_stride(shard, block) if wire_stride is None else wire_stride
    sw = qr.wire_bytes(shard, block)
    wbytes, ebytes = (n - 1) * stride + sw, n * shard * item
    vp, ep = shard_input(layout, n, shard, block, dtype)
    want = shard_expectation(layout, n, shard, block, dtype, use_err)
    arena = sr.Arena(counts, dtype, misalign)

    in_img = arena.fill(vp[:total])
    d_in = api.put(in_img)
    tensors = [d_in[s:s + c * item] for s, c in zip(arena.starts, counts)]
    wire_img, lo = sr.guarded_bytes(wbytes, 0xAB)
    err_img, _ = sr.guarded_bytes(ebytes, ep.view(np.uint8))
    d_wire, d_err = api.put(wire_img), api.put(err_img)
    api.quantize_gather_shards(tensors, counts, d_wire[lo:lo + wbytes], n, shard,
                               d_err[lo:lo + ebytes] if use_err else None, block, dtype,
                               wire_stride)
    h_wire, h_err = api.get(d_wire), api.get(d_err)
    wire = h_wire[lo:lo + wbytes]
    err = h_err[lo:lo + ebytes].view(BITS[dtype])
    h_in = api.get(d_in)
    assert np.array_equal(h_in, in_img), "quantize_gather_shards wrote to its input"
    assert arena.guards_intact(h_in), "the tensors' arena guards"
    assert sr.body_intact(h_wire, wbytes) and sr.body_intact(h_err, ebytes), \
        "write outside the wire or the residual"
    for j in range(n):
        what = f"shard {j}"
        got = wire[j * stride:j * stride + sw]
        scales, word1, q = qr.parse_wire(got, block)
        assert np.array_equal(scales.view(np.uint32), want[j]["scales"].view(np.uint32)), \
            f"{what}: scales"
        assert not word1.view(np.uint32).any(), f"{what}: reserved header word"
        assert np.array_equal(q, want[j]["q"]), f"{what}: payload (padding included)"
        assert np.array_equal(got, want[j]["wire"]), what
        gap = wire[j * stride + sw:(j + 1) * stride]
        assert (gap == 0xAB).all(), f"{what}: bytes between two shards' wires written"
        e = err[j * shard:(j + 1) * shard]
        if use_err:
            ok = sr.residual_ok(e, want[j])
            assert ok.all(), f"{what} residual: {(~ok).sum()} elements match neither rounding"
    if use_err:
        assert not err[total:].any(), "a padding element's residual is not +0"
    else:
        assert np.array_equal(err, ep.view(BITS[dtype])), "residual written without err"

    # the flat codec of the same api, launched per shard on the materialised V'
    f_in = api.put(np.ascontiguousarray(vp).view(np.uint8))
    f_wire = api.put(np.full(wbytes, 0xAB, dtype=np.uint8))
    f_err = api.put(np.ascontiguousarray(ep).view(np.uint8))
    sb = shard * item
    for j in range(n):
        api.quantize(f_in[j * sb:(j + 1) * sb], f_wire[j * stride:j * stride + sw], shard,
                     f_err[j * sb:(j + 1) * sb] if use_err else None, block, dtype)
    assert np.array_equal(api.get(f_wire), wire), "differs from the flat quantize's wires"
    assert np.array_equal(api.get(f_err).view(BITS[dtype]), err), \
        "differs from the flat quantize's residual"

    if n == 1:
        # one shard of exactly the concatenation: quantize_gather's bytes
        assert shard == total
        g_wire = api.put(np.full(sw, 0xAB, dtype=np.uint8))
        g_err = api.put(np.ascontiguousarray(ep).view(np.uint8))
        api.quantize_gather(tensors, counts, g_wire, g_err if use_err else None, block, dtype)
        assert np.array_equal(api.get(g_wire), wire[:sw]), "differs from quantize_gather's wire"
        assert np.array_equal(api.get(g_err).view(BITS[dtype]), err), \
            "differs from quantize_gather's residual"
    return dict(wire=wire.copy(), err=err.copy())


def residual_forms_agree(layout, n, shard, block, dtype):
    """Per element of V': whether the two allowed roundings of the residual are
    the same bits (there the kernel and its twin must agree too)."""
    want = shard_expectation(layout, n, shard, block, dtype, True)
    return np.concatenate([x["err_unfused"].view(BITS[dtype]) == x["err_fused"].view(BITS[dtype])
                           for x in want])


# ---- launcher --------------------------------------------------------------

def run_ranks(worker, world, device=False, timeout=120, extra_env=None, **kwargs):
    """tests.workers_quant_rs_seg.<worker>(**kwargs) in `world` processes, on
    the TCP transport or (device=True) all on GPU 0. Every process gets
    `timeout` seconds; the first to exceed it takes all ranks down. Raises on a
    nonzero exit; returns the stdouts."""
    port = free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ)
        env.pop("MLSL_QUANT_RS_ALGO", None)
        env.update({"RANK": str(r), "WORLD_SIZE": str(world),
                    "MASTER_ADDR": "127.0.0.1", "MLSL_PORT": str(port),
                    "PYTHONPATH": REPO, "QRS_DEVICE": w.qrs_device(device)})
        if device:
            env.pop("MLSL_TRANSPORT", None)
            env["MLSL_TIMEOUT"] = "90"
        else:
            env["MLSL_TRANSPORT"] = "tcp"
        if extra_env:
            env.update(extra_env)
        procs.append(subprocess.Popen(
            [sys.executable, "-m", "tests.workers_quant_rs_seg", worker, json.dumps(kwargs)],
            env=env, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
            text=True))
    outs, failed = [], []
    for r, p in enumerate(procs):
        try:
            out, _ = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            for q in procs:
                q.wait()
            raise AssertionError(f"rank {r} timed out ({worker} world={world})")
        outs.append(out)
        if p.returncode != 0:
            failed.append((r, p.returncode, out))
    if failed:
        msgs = "\n".join(f"--- rank {r} rc={rc} ---\n{out[-3000:]}" for r, rc, out in failed)
        raise AssertionError(f"{worker} world={world} failed:\n{msgs}")
    return outs


def assert_all_checked(outs, world):
    """Every rank printed how many starts it compared, and compared some."""
    for r, out in enumerate(outs):
        lines = [l for l in out.splitlines() if l.startswith("CHECKED ")]
        assert len(lines) == 1 and int(lines[0].split()[1]) > 0, (r, out[-500:])
    assert len(outs) == world


# ---- workers ---------------------------------------------------------------

STARTS = 3
# (counts, shard or None for the default): the edge layout, about 3 MiB of f32
# in ragged tensors, five elements (at four ranks the last one owns nothing but
# padding), and a shard larger than it has to be
COLL_CASES = {
    "edges": (sr.LAYOUTS["edges"], None),
    "ragged3m": (sr.RAGGED_3MIB, None),
    "five": ([2, 3], None),
    "edges_wide": (sr.LAYOUTS["edges"], 1284 + 130),
}
# with a block of 12 elements a wire block is 20 bytes: one block per shard at
# every world, so a shard's wire, the plan's stride, is no multiple of 8
ODD_WIRE_BLOCK = 12
ODD_WIRE_CASES = {"tiny24": ([10, 14], None), "edges": (sr.LAYOUTS["edges"], None)}
# codec cases whose shard has an odd number of wire blocks of 4 (mod 8) bytes:
# (layout, N, shard, block), run at a stride of exactly one shard's wire
ODD_WIRE_SHARD_CASES = [("edges", 4, 513, 12), ("edges", 3, 428, 100)]


def _run_pair(mx, bufs, d, rank, size, counts, shard, dtype, algo, ref_algo):
    """STARTS starts of one SegmentedReduceScatter and of one flat quantized
    reduce_scatter on the materialised V'; recv must hold the same bits. Both
    requests carry their residual from start to start. The tensors and recv of
    every start are new allocations, the earlier ones still alive, so that
    their addresses differ. Returns the results' bytes."""
    total = sum(counts)
    offs = sr.offsets(counts)
    req = mx.SegmentedReduceScatter(d, counts, shard=shard, dtype=dtype, group="data",
                                    algo=algo)
    want_shard = (total + size - 1) // size if shard is None else shard
    assert req.shard == want_shard, (req.shard, want_shard)
    shard = req.shard
    ref = mx.PersistentRequest(d, "reduce_scatter", shard, dtype=dtype, op="sum", group="data",
                               quantized=True, algo=ref_algo)
    keep, results = [], []
    for s in range(STARTS):
        x = ws.start_input(rank, s, total, dtype)
        vp = np.concatenate([x, np.zeros(size * shard - total, dtype=x.dtype)])
        flat, f_recv = bufs.put(vp), bufs.put(np.full(shard, 0x4141, dtype=BITS[dtype])
                                              .view(NP_DT[dtype]))
        ref.start(flat, f_recv)
        ref.wait()
        want = bufs.get(f_recv, dtype).view(BITS[dtype])
        tensors = [bufs.put(x[offs[j]:offs[j + 1]]) for j in range(len(counts))]
        recv = bufs.put(np.full(shard, 0x4242, dtype=BITS[dtype]).view(NP_DT[dtype]))
        keep.append((tensors, recv))
        req.start(tensors, recv)
        assert req.test() in (True, False)
        req.wait()
        got = bufs.get(recv, dtype).view(BITS[dtype])
        bad = int((got != want).sum())
        what = (size, dtype, algo, len(counts), total, shard, f"start {s}")
        assert bad == 0, (what, f"{bad} of {shard} elements differ from the flat request")
        back = np.concatenate([bufs.get(t, dtype) for t in tensors]).view(BITS[dtype])
        assert np.array_equal(back, x.view(BITS[dtype])), (what, "a tensor was written")
        results.append(got.tobytes())
    req.destroy()
    ref.destroy()
    return results


def rs_seg_check(algos=("ring", "direct"), dtypes=("f32", "bf16"), cases=None, block=None):
    """Every configuration of _run_pair at this world size. `block` sets the
    quantization block (ODD_WIRE_BLOCK runs ODD_WIRE_CASES)."""
    mx, bufs, rank, size = w._init()
    d = mx.Distribution(size, 1)
    table = COLL_CASES
    if block is not None:
        assert block == ODD_WIRE_BLOCK
        mx.set_quant_params(block)
        table = ODD_WIRE_CASES
    checked = 0
    for name in cases or list(table):
        counts, shard = table[name]
        if shard is not None:
            shard = (shard + size - 1) // size
        for algo in algos:
            for dtype in dtypes:
                checked += len(_run_pair(mx, bufs, d, rank, size, counts, shard, dtype, algo,
                                         algo))
    print(f"CHECKED {checked}")
    d.barrier("global")
    mx.finalize()


def rs_seg_env_algo(env_algo="direct"):
    """algo=None takes MLSL_QUANT_RS_ALGO (set by the launcher): the result is
    the flat request's with that algorithm NAMED, and at three ranks and more
    it is not the other algorithm's."""
    mx, bufs, rank, size = w._init()
    assert os.environ.get("MLSL_QUANT_RS_ALGO") == env_algo
    d = mx.Distribution(size, 1)
    counts = sr.LAYOUTS["edges"]
    got = _run_pair(mx, bufs, d, rank, size, counts, None, "f32", None, env_algo)
    other = "ring" if env_algo == "direct" else "direct"
    oth = _run_pair(mx, bufs, d, rank, size, counts, None, "f32", other, other)
    if size >= 3:
        assert got != oth, "both algorithms gave the same bits: the case proves nothing"
    d.barrier("global")
    mx.finalize()


def _last_error():
    import ctypes
    from mlsl_amd._lib import lib
    return ctypes.string_at(lib().mlsl_last_error()).decode()


def rs_seg_refusals():
    """What creation and start refuse, by message; a refused start leaves the
    request usable."""
    import ctypes
    mx, bufs, rank, size = w._init()
    from mlsl_amd._lib import check, lib
    L = lib()
    raises = ws._raises
    d = mx.Distribution(size, 1)
    mk = lambda counts, **kw: (lambda: mx.SegmentedReduceScatter(d, counts, group="data", **kw))
    what = "reduce_scatter over a tensor list"
    raises(RuntimeError, f"{what} supports f32/bf16 only", mk([4, 4], dtype="f64"))
    raises(RuntimeError, f"{what} supports f32/bf16 only", mk([4, 4], dtype="f16"))
    raises(RuntimeError, f"{what} needs at least one tensor (nseg == 0)", mk([]))
    raises(RuntimeError, f"{what}: tensor 1 has a zero count", mk([4, 0, 4]))
    raises(RuntimeError, f"{what}: shard * N < total", mk([40, 40], shard=1))
    raises(ValueError, "algo", mk([4], algo="two_shot"))
    if size > 8:
        raises(RuntimeError, "direct quantized reduce_scatter supports at most 8 ranks",
               mk([4, 4], algo="direct"))
        mk([4, 4], algo="ring")().destroy()
    req = mk([3, 5], dtype="f32")()
    assert req.shard == (8 + size - 1) // size
    zero = mk([3, 5], shard=0)()
    assert zero.shard == req.shard, "shard=0 is the default, and .shard says which"
    zero.destroy()
    a, b = bufs.put(np.ones(3, F32)), bufs.put(np.ones(5, F32))
    recv = bufs.put(np.zeros(req.shard, F32))
    raises(RuntimeError, "nseg differs from creation", lambda: req.start([a], recv))
    raises(RuntimeError, "nseg differs from creation", lambda: req.start([a, b, b], recv))
    raises(RuntimeError, "tensor 1 is null", lambda: req.start([a, 0], recv))
    raises(RuntimeError, "tensor 0 is null", lambda: req.start([None, b], recv))
    raises(RuntimeError, "recv is null", lambda: req.start([a, b], None))
    if bufs.gpu:
        raises(RuntimeError, "reduce_scatter start over a tensor list: tensor 1 is not device "
               "memory", lambda: req.start([a, np.ones(5, F32)], recv))
        raises(RuntimeError, "reduce_scatter start over a tensor list: recv is not device "
               "memory", lambda: req.start([a, b], np.zeros(req.shard, F32)))
    # neither of the other two starts is this request's
    assert L.mlsl_request_start(req._h, None, None) != 0
    assert "mlsl_request_start_segments_recv" in _last_error()
    L.mlsl_request_start_segments.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p),
                                              ctypes.c_size_t]
    assert L.mlsl_request_start_segments(req._h, req._ptrs, 2) != 0
    assert "mlsl_request_start_segments_recv" in _last_error()
    # and its start is no other request's
    flat = mx.PersistentRequest(d, "reduce_scatter", 4, dtype="f32", op="sum", group="data",
                                quantized=True)
    ar = mx.SegmentedAllReduce(d, [3, 5], dtype="f32", group="data")
    for other in (flat, ar):
        raises(RuntimeError, "not described as a reduce_scatter over a tensor list",
               lambda: check(L.mlsl_request_start_segments_recv(
                   other._h, req._ptrs, 2, ctypes.c_void_p(0))))
    flat.destroy()
    ar.destroy()
    req.start([a, b], recv)
    req.wait()
    lo = rank * req.shard
    want = np.where(np.arange(lo, lo + req.shard) < 8, float(size), 0.0)
    assert np.allclose(bufs.get(recv, "f32"), want, rtol=0.02, atol=0)
    req.destroy()
    d.barrier("global")
    mx.finalize()


def rs_seg_plugin():
    """With a compression plugin the request fails at creation: the plugin
    ABI quantizes one flat buffer. Direct keeps its own message."""
    import ctypes
    from ctypes import byref, c_char_p, c_size_t, c_void_p
    assert os.path.exists(w.PLUGIN), "build the plugin first: ensure_plugin()"
    mx, bufs, rank, size = w._init()
    from mlsl_amd._lib import lib
    L = lib()

    class QP(ctypes.Structure):
        _fields_ = [("lib_path", c_char_p), ("quant", c_char_p),
                    ("dequant", c_char_p), ("reduce_sum", c_char_p),
                    ("block_size", c_size_t), ("elem_in_block", c_size_t)]

    env = c_void_p()
    assert L.mlsl_environment_get_env(byref(env)) == 0
    assert L.mlsl_environment_set_quantization_params(
        env, byref(QP(w.PLUGIN.encode(), None, None, None, 264, 256))) == 0, _last_error()
    d = mx.Distribution(size, 1)
    ws._raises(RuntimeError, "reduce_scatter over a tensor list cannot run with a compression "
               "plugin (the plugin ABI quantizes one flat buffer)",
               lambda: mx.SegmentedReduceScatter(d, [5, 7], group="data", algo="ring"))
    ws._raises(RuntimeError, "direct quantized reduce_scatter cannot run with a compression "
               "plugin", lambda: mx.SegmentedReduceScatter(d, [5, 7], group="data",
                                                           algo="direct"))
    L.mlsl_environment_set_quantization_params(
        env, byref(QP(None, None, None, None, 0, 256)))
    d.barrier("global")
    mx.finalize()


def _net(torch):
    class Net(torch.nn.Module):
        """1245 parameters, odd, so every world pads; `unused` never gets a
        gradient."""

        def __init__(self):
            super().__init__()
            self.w1 = torch.nn.Parameter(torch.randn(7, 5))
            self.b1 = torch.nn.Parameter(torch.randn(7))
            self.unused = torch.nn.Parameter(torch.randn(3))
            self.w2 = torch.nn.Parameter(torch.randn(300, 3))
            self.b2 = torch.nn.Parameter(torch.randn(300))

        def forward(self, x):
            h = torch.tanh(x @ self.w1.t() + self.b1)
            return (h[:, :3] @ self.w2.t() + self.b2).square().mean()

    return Net()


def zero1_check(rs_algo="ring", ag_compression="none"):
    """ShardedOptimizer(grads="in_place") against grads="copy" from the same
    seeds: three steps of SGD with momentum, the parameters' bits identical
    after every step. One parameter's grad stays None, and in the second step
    one gradient is handed over non-contiguous."""
    mx, bufs, rank, size = w._init()
    import torch
    from mlsl_amd.parallel.zero1 import ShardedOptimizer
    dev = "cuda" if bufs.gpu else "cpu"
    d = mx.Distribution(size, 1)
    models, opts = [], []
    for grads in ("copy", "in_place"):
        torch.manual_seed(11)
        m = _net(torch).to(dev)
        models.append(m)
        opts.append(ShardedOptimizer(m.parameters(), torch.optim.SGD, d, reduce="rs",
                                     compression="int8", rs_algo=rs_algo,
                                     ag_compression=ag_compression, grads=grads, lr=0.05,
                                     momentum=0.9))
    copy, inp = opts
    assert copy.shard * size > 1245, "no padding: the case proves nothing"
    assert hasattr(copy, "flat_grad") and copy.flat_grad.numel() == copy.shard * size
    assert not hasattr(inp, "flat_grad"), "in_place kept the model-sized gradient buffer"
    assert inp.own_grad.numel() == inp.shard == copy.shard
    assert inp.own_grad.untyped_storage().nbytes() == inp.shard * inp.own_grad.element_size()
    assert torch.equal(copy.flat, inp.flat)
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
        if bufs.gpu:
            torch.cuda.synchronize()
        a = copy.flat.detach().cpu().view(torch.int32).numpy()
        b = inp.flat.detach().cpu().view(torch.int32).numpy()
        bad = int((a != b).sum())
        assert bad == 0, (it, rs_algo, ag_compression, f"{bad} of {a.size} parameters differ")
        assert np.abs(copy.flat.detach().cpu().numpy()).sum() > 0
    assert list(inp._zero_grads) == [2], "one cached zero gradient, for `unused`"
    print(f"CHECKED {3}")
    d.barrier("global")
    mx.finalize()


def zero1_refusals():
    """grads="in_place" without reduce="rs" or without int8, and an unknown
    value, by message; at world 1 it changes nothing."""
    mx, bufs, rank, size = w._init()
    import torch
    from mlsl_amd.parallel.zero1 import ShardedOptimizer
    d = mx.Distribution(size, 1)
    mk = lambda **kw: (lambda: ShardedOptimizer(_net(torch).parameters(), torch.optim.SGD, d,
                                                lr=0.1, **kw))
    ws._raises(ValueError, 'it needs reduce="rs"', mk(grads="in_place"))
    ws._raises(ValueError, 'it needs reduce="rs"',
               mk(grads="in_place", reduce="none", compression="none"))
    ws._raises(ValueError, 'it needs compression="int8"', mk(grads="in_place", reduce="rs"))
    ws._raises(ValueError, "expected 'copy' or 'in_place'",
               mk(grads="views", reduce="rs", compression="int8"))
    if size == 1:
        o = mk(grads="in_place", reduce="rs", compression="int8")()
        assert hasattr(o, "flat_grad") and o._qrs_seg is None
    d.barrier("global")
    mx.finalize()


WORKERS = {
    "rs_seg_check": rs_seg_check,
    "rs_seg_env_algo": rs_seg_env_algo,
    "rs_seg_refusals": rs_seg_refusals,
    "rs_seg_plugin": rs_seg_plugin,
    "zero1_check": zero1_check,
    "zero1_refusals": zero1_refusals,
}


def main():
    name = sys.argv[1]
    kwargs = json.loads(sys.argv[2]) if len(sys.argv) > 2 else {}
    WORKERS[name](**kwargs)
    print(f"OK {name} rank={os.environ.get('RANK')}")


if __name__ == "__main__":
    main()
