"""The quantized allreduce over a list of tensors: what its tests share, and
their rank workers.

Codec cases run through `run_codec_case` with an `api` object that says where
the bytes live (numpy for the host twins, torch on GPU 0 for the kernels).
Collective workers compare every start of a `SegmentedAllReduce` with the
existing flat quantized `PersistentRequest` on the materialised
concatenation, scaled by post_scale in float32 numpy: same wire, same
residual, so the bits must agree. Transport: TCP with numpy buffers, or every
rank on GPU 0 with torch buffers (QRS_DEVICE picks, as in workers_quant_rs).

Run as: python -m tests.workers_quant_seg <worker> '<json kwargs>'
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

from tests import quant_ref as qr
from tests import quant_seg_ref as sr
from tests import workers_quant_rs as w
from tests.mp import REPO, free_port

F32 = np.float32
ITEM, NP_DT, BITS = sr.ITEM, sr.NP_DT, sr.BITS


# ---- codec cases -----------------------------------------------------------

class HostApi:
    """The host twins on numpy bytes."""

    def put(self, img):
        a = sr.aligned_bytes(img.size)
        a[:] = img
        return a

    def get(self, buf):
        return np.array(buf, copy=True)

    def quantize_gather(self, tensors, counts, wire, err, block, dtype):
        from mlsl_amd import ops
        ops.host_quantize_gather(tensors, counts, wire, err=err, block=block, dtype=dtype)

    def dequantize_scatter(self, wire, tensors, counts, block, dtype, post_scale,
                           round_first=False):
        from mlsl_amd import ops
        ops.host_dequantize_scatter(wire, tensors, counts, block=block, dtype=dtype,
                                    post_scale=post_scale, round_first=round_first)

    def quantize(self, inp, wire, count, err, block, dtype):
        from mlsl_amd import ops
        ops.host_quantize(inp, wire, count, err=err, block=block, dtype=dtype)

    def dequantize(self, wire, out, count, block, dtype):
        from mlsl_amd import ops
        ops.host_dequantize(wire, out, count, block=block, dtype=dtype)


def run_codec_case(api, layout, block, dtype, use_err, misalign):
    """quantize_gather, then dequantize_scatter at every post_scale, of one
    layout through `api`, against the numpy reference and against the flat
    codec of the same `api` on the materialised concatenation. Bit for bit;
    the residual also has to be one of the two roundings quant_ref allows.
    Sentinels around the wire, the residual and every tensor must survive,
    and what is only read must not change. Returns dict(wire, err, outs)."""
    counts = sr.LAYOUTS[layout]
    count, item = sum(counts), ITEM[dtype]
    nbytes, wbytes = count * item, qr.wire_bytes(count, block)
    v, e0 = sr.case_input(layout, block, dtype)
    want = sr.gather_expectation(layout, block, dtype, use_err)
    arena = sr.Arena(counts, dtype, misalign)

    def tensors_of(buf):
        return [buf[s:s + n * item] for s, n in zip(arena.starts, counts)]

    in_img = arena.fill(v)
    d_in = api.put(in_img)
    wire_img, lo = sr.guarded_bytes(wbytes, 0xAB)
    err_img, _ = sr.guarded_bytes(nbytes, e0.view(np.uint8))
    d_wire, d_err = api.put(wire_img), api.put(err_img)
    api.quantize_gather(tensors_of(d_in), counts, d_wire[lo:lo + wbytes],
                        d_err[lo:lo + nbytes] if use_err else None, block, dtype)
    h_wire, h_err = api.get(d_wire), api.get(d_err)
    wire = h_wire[lo:lo + wbytes]
    err = h_err[lo:lo + nbytes].view(BITS[dtype])
    assert np.array_equal(api.get(d_in), in_img), "quantize_gather wrote to its input"
    assert sr.body_intact(h_wire, wbytes) and sr.body_intact(h_err, nbytes), \
        "write outside the wire or the residual"
    scales, word1, q = qr.parse_wire(wire, block)
    assert np.array_equal(scales.view(np.uint32), want["scales"].view(np.uint32)), "scales"
    assert not word1.view(np.uint32).any(), "reserved header word"
    assert np.array_equal(q, want["q"]), "payload (padding included)"
    assert np.array_equal(wire, want["wire"])
    assert scales[qr.TIE_BLOCK] == F32(0.125) and scales[qr.ZERO_BLOCK] == 1.0
    if use_err:
        ok = sr.residual_ok(err, want)
        assert ok.all(), f"residual: {(~ok).sum()} elements match neither rounding"
    else:
        assert np.array_equal(err, e0.view(BITS[dtype])), "residual written without err"

    # the flat codec of the same api on the materialised concatenation
    f_in = api.put(np.ascontiguousarray(v).view(np.uint8))
    f_wire = api.put(np.full(wbytes, 0xAB, dtype=np.uint8))
    f_err = api.put(np.ascontiguousarray(e0).view(np.uint8))
    f_out = api.put(np.full(nbytes, 0xAB, dtype=np.uint8))
    api.quantize(f_in, f_wire, count, f_err if use_err else None, block, dtype)
    api.dequantize(f_wire, f_out, count, block, dtype)
    assert np.array_equal(api.get(f_wire), wire), "differs from the flat quantize's wire"
    assert np.array_equal(api.get(f_err).view(BITS[dtype]), err), \
        "differs from the flat quantize's residual"
    flat_out = api.get(f_out).view(BITS[dtype])

    outs, visible, rf_visible = {}, 0, 0
    for rf in (False, True):
        for ps in sr.POST_SCALES:
            what = f"post_scale {ps} round_first {rf}"
            d_out = api.put(arena.blank())
            api.dequantize_scatter(d_wire[lo:lo + wbytes], tensors_of(d_out), counts, block,
                                   dtype, ps, round_first=rf)
            h_out = api.get(d_out)
            assert arena.guards_intact(h_out), f"{what}: write outside the tensors"
            got = arena.gather(h_out).view(BITS[dtype])
            ref = sr.ref_dequantize_scatter(want["wire"], count, block, dtype, ps,
                                            round_first=rf).view(BITS[dtype])
            bad = int((got != ref).sum())
            assert bad == 0, f"{what}: {bad} of {count} elements differ"
            if ps == 1.0:
                assert np.array_equal(got, flat_out), f"{what} differs from the flat dequantize"
            elif not rf:
                one = sr.ref_dequantize_fused_scale(want["wire"], count, block, dtype, ps)
                visible += int((one.view(BITS[dtype]) != ref).sum())
            if rf:
                # the flat dequantize's stored elements, scaled in float32
                scaled = qr.encode((qr.decode(flat_out.view(NP_DT[dtype]), dtype) * F32(ps))
                                   .astype(F32), dtype).view(BITS[dtype])
                assert np.array_equal(got, scaled), f"{what}: not the flat result scaled"
                rf_visible += int((got != outs[(ps, False)]).sum())
            outs[(ps, rf)] = got
    # rounding first changes nothing for f32, and bf16 at a third
    assert (rf_visible > 0) == (dtype == "bf16"), rf_visible
    h_wire2 = api.get(d_wire)
    assert np.array_equal(h_wire2, h_wire), "dequantize_scatter wrote to the wire"
    if dtype == "f32":
        assert visible > 0, "no element shows the two roundings: the case proves nothing"
    return dict(wire=wire.copy(), err=err.copy(), outs=outs)


CODEC_PARAMS = [(layout, block, dtype, use_err, misalign)
                for layout in sr.LAYOUTS for block in sr.BLOCKS for dtype in ("f32", "bf16")
                for use_err in (True, False) for misalign in (False, True)]


def codec_id(p):
    layout, block, dtype, use_err, misalign = p
    return f"{layout}-{block}-{dtype}-{'err' if use_err else 'noerr'}-" \
           f"{'off1' if misalign else 'al16'}"


# ---- launcher --------------------------------------------------------------

def run_ranks(worker, world, device=False, timeout=120, extra_env=None, **kwargs):
    """tests.workers_quant_seg.<worker>(**kwargs) in `world` processes, on the
    TCP transport or (device=True) all on GPU 0. Every process gets `timeout`
    seconds; the first to exceed it takes all ranks down. Raises on a nonzero
    exit; returns the stdouts."""
    port = free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ)
        env.pop("MLSL_QUANT_AR_ALGO", None)
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
            [sys.executable, "-m", "tests.workers_quant_seg", worker, json.dumps(kwargs)],
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


def assert_ranks_agree(outs, world):
    """Every rank printed the same digests, at least one."""
    found = {}
    for out in outs:
        for line in out.splitlines():
            if line.startswith("DIGEST "):
                _, r, h = line.split()
                found.setdefault(int(r), []).append(h)
    assert sorted(found) == list(range(world)), sorted(found)
    assert found[0] and all(v == found[0] for v in found.values()), \
        "results differ across ranks"


# ---- workers ---------------------------------------------------------------

STARTS = 3


def start_input(rank, start, count, dtype):
    """Rank `rank`'s concatenation for start number `start`."""
    rng = np.random.default_rng(7000 + 97 * rank + start)
    return qr.encode((rng.standard_normal(count) * 3).astype(F32), dtype)


def _post_scales(size):
    return [1.0] if size == 1 else [1.0, 1.0 / size]


def _run_pair(mx, bufs, d, rank, size, counts, dtype, ar_algo, ref_algo, post_scale):
    """STARTS starts of one SegmentedAllReduce and of one flat quantized
    PersistentRequest on the same data; every tensor must hold the flat
    result times post_scale (float32, rounded to the dtype), bit for bit.
    Both requests carry their residual from start to start. The tensors of
    every start are new allocations, the earlier ones still alive, so that
    their addresses differ. Returns the results' bytes."""
    count = sum(counts)
    offs = sr.offsets(counts)
    req = mx.SegmentedAllReduce(d, counts, dtype=dtype, group="data", ar_algo=ar_algo,
                                post_scale=post_scale)
    ref = mx.PersistentRequest(d, "all_reduce", count, dtype=dtype, op="sum", group="data",
                               quantized=True, ar_algo=ref_algo)
    keep, results = [], []
    for s in range(STARTS):
        x = start_input(rank, s, count, dtype)
        flat = bufs.put(x)
        ref.start(flat, flat)
        ref.wait()
        want = qr.encode((qr.decode(bufs.get(flat, dtype), dtype) * F32(post_scale))
                         .astype(F32), dtype).view(BITS[dtype])
        tensors = [bufs.put(x[offs[j]:offs[j + 1]]) for j in range(len(counts))]
        keep.append(tensors)
        req.start(tensors)
        assert req.test() in (True, False)
        req.wait()
        got = np.concatenate([bufs.get(t, dtype) for t in tensors]).view(BITS[dtype])
        bad = int((got != want).sum())
        what = (size, dtype, ar_algo, post_scale, len(counts), count, f"start {s}")
        assert bad == 0, (what, f"{bad} of {count} elements differ from the flat request")
        results.append(got.tobytes())
    req.destroy()
    ref.destroy()
    return results


def seg_check(algos=("ring", "two_shot"), dtypes=("f32", "bf16"), layouts=None,
              inv_world=None):
    """Every configuration of _run_pair at this world size; one digest per
    configuration for the launcher's cross-rank comparison. `inv_world`
    narrows post_scale to 1 (False) or 1/world (True)."""
    mx, bufs, rank, size = w._init()
    d = mx.Distribution(size, 1)
    scales = _post_scales(size) if inv_world is None else [1.0 / size if inv_world else 1.0]
    for name in layouts or list(sr.COLL_LAYOUTS):
        for algo in algos:
            for dtype in dtypes:
                for ps in scales:
                    res = _run_pair(mx, bufs, d, rank, size, sr.COLL_LAYOUTS[name], dtype,
                                    algo, algo, ps)
                    h = hashlib.sha256(b"".join(res)).hexdigest()
                    print(f"DIGEST {rank} {h}")
    d.barrier("global")
    mx.finalize()


def seg_env_algo(env_algo="two_shot"):
    """ar_algo=None takes MLSL_QUANT_AR_ALGO (set by the launcher): the result
    is the flat request's with that algorithm NAMED, and at three ranks and
    more it is not the other algorithm's."""
    mx, bufs, rank, size = w._init()
    assert os.environ.get("MLSL_QUANT_AR_ALGO") == env_algo
    d = mx.Distribution(size, 1)
    counts = sr.COLL_LAYOUTS["edges"]
    got = _run_pair(mx, bufs, d, rank, size, counts, "f32", None, env_algo, 1.0)
    other = "ring" if env_algo == "two_shot" else "two_shot"
    oth = _run_pair(mx, bufs, d, rank, size, counts, "f32", other, other, 1.0)
    if size >= 3:
        assert got != oth, "both algorithms gave the same bits: the case proves nothing"
    d.barrier("global")
    mx.finalize()


def _raises(exc, needle, f):
    try:
        f()
    except exc as e:
        assert needle in str(e), (needle, str(e))
        return True
    raise AssertionError(f"no {exc.__name__} with {needle!r}")


def seg_refusals():
    """What creation and start refuse, by message; a refused start leaves the
    request usable."""
    mx, bufs, rank, size = w._init()
    d = mx.Distribution(size, 1)
    mk = lambda counts, **kw: (lambda: mx.SegmentedAllReduce(d, counts, group="data", **kw))
    _raises(RuntimeError, "f32/bf16 only", mk([4, 4], dtype="f64"))
    _raises(RuntimeError, "f32/bf16 only", mk([4, 4], dtype="f16"))
    _raises(RuntimeError, "nseg == 0", mk([]))
    _raises(RuntimeError, "tensor 1 has a zero count", mk([4, 0, 4]))
    _raises(ValueError, "ar_algo", mk([4], ar_algo="direct"))
    if size > 8:
        _raises(RuntimeError, "at most 8 ranks", mk([4, 4], ar_algo="two_shot"))
        mk([4, 4], ar_algo="ring")().destroy()
    req = mk([3, 5], dtype="f32")()
    a, b = bufs.put(np.ones(3, F32)), bufs.put(np.ones(5, F32))
    _raises(RuntimeError, "nseg differs from creation", lambda: req.start([a]))
    _raises(RuntimeError, "nseg differs from creation", lambda: req.start([a, b, b]))
    if bufs.gpu:
        host = np.ones(5, F32)
        _raises(RuntimeError, "tensor 1 is not device memory", lambda: req.start([a, host]))
    # the flat start is not this request's
    from mlsl_amd._lib import lib
    assert lib().mlsl_request_start(req._h, None, None) != 0
    req.start([a, b])
    req.wait()
    assert np.allclose(bufs.get(a, "f32"), size, rtol=0.02)
    assert np.allclose(bufs.get(b, "f32"), size, rtol=0.02)
    req.destroy()
    d.barrier("global")
    mx.finalize()


def seg_plugin():
    """With a compression plugin the request fails at creation: the plugin
    ABI quantizes one flat buffer. Two-shot keeps its own message."""
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
        env, byref(QP(w.PLUGIN.encode(), None, None, None, 264, 256))) == 0, \
        ctypes.string_at(L.mlsl_last_error()).decode()
    d = mx.Distribution(size, 1)
    _raises(RuntimeError, "plugin ABI quantizes one flat buffer",
            lambda: mx.SegmentedAllReduce(d, [5, 7], group="data", ar_algo="ring"))
    _raises(RuntimeError, "use the ring",
            lambda: mx.SegmentedAllReduce(d, [5, 7], group="data", ar_algo="two_shot"))
    L.mlsl_environment_set_quantization_params(
        env, byref(QP(None, None, None, None, 0, 256)))
    d.barrier("global")
    mx.finalize()


def _mlp(torch, with_f64):
    class Net(torch.nn.Module):
        """Weights 7x5 and 300x3 with biases; optionally one f64 parameter."""

        def __init__(self):
            super().__init__()
            self.w1 = torch.nn.Parameter(torch.randn(7, 5))
            self.b1 = torch.nn.Parameter(torch.randn(7))
            self.w2 = torch.nn.Parameter(torch.randn(300, 3))
            self.b2 = torch.nn.Parameter(torch.randn(300))
            if with_f64:
                self.s = torch.nn.Parameter(torch.randn(3, dtype=torch.float64))

        def forward(self, x):
            h = torch.tanh(x @ self.w1.t() + self.b1)
            y = (h[:, :3] @ self.w2.t() + self.b2).sum()
            if with_f64:
                y = y.double() * self.s.sum() + (self.s * self.s).sum()
            return y

    return Net()


def ddp_check(with_f64=False, ar_algo=None):
    """DistributedData(compression="int8") against a flat quantized request
    per bucket fed with torch.cat of the same local gradients (computed on a
    twin model), scaled by 1/world: every p.grad bit for bit, over three
    iterations with zero_grad(set_to_none=True), the reference's residual
    carried as DDP's is. An f64 bucket takes the exact path and matches the
    manual average."""
    mx, bufs, rank, size = w._init()
    import torch
    from mlsl_amd.parallel import DistributedData
    dev = "cuda" if bufs.gpu else "cpu"
    torch.manual_seed(11)
    model, twin = _mlp(torch, with_f64).to(dev), _mlp(torch, with_f64).to(dev)
    d = mx.Distribution(size, 1)
    dd = DistributedData(model, dist=d, bucket_mb=0.003, compression="int8", ar_algo=ar_algo)
    twin.load_state_dict(model.state_dict())
    names = {id(p): n for n, p in model.named_parameters()}
    tw = dict(twin.named_parameters())
    buckets = [[names[id(p)] for p in ps] for ps in dd._buckets]
    quant = [tw[b[0]].dtype == torch.float32 for b in buckets]
    assert sum(quant) == 2, buckets
    assert len(buckets) == (3 if with_f64 else 2), buckets
    assert [r is not None for r in dd._seg] == quant
    refs = [mx.PersistentRequest(d, "all_reduce", sum(tw[n].numel() for n in b), dtype="f32",
                                 op="sum", group="data", quantized=True, ar_algo=ar_algo)
            if qz else None for b, qz in zip(buckets, quant)]
    ps = F32(1.0 / size)
    for it in range(3):
        xs = [torch.randn(6, 5, generator=torch.Generator().manual_seed(300 + it * size + r))
              for r in range(size)]
        twin.zero_grad(set_to_none=True)
        twin(xs[rank].to(dev)).backward()
        want = {}
        for b, qz, ref in zip(buckets, quant, refs):
            flat = torch.cat([tw[n].grad.detach().reshape(-1) for n in b])
            if qz:
                ref.start(flat, flat)
                ref.wait()
                if bufs.gpu:
                    torch.cuda.synchronize()
                red = (flat.cpu().numpy() * ps).astype(F32)
            else:
                mx.wait(d.all_reduce(flat, flat, flat.numel(), op="sum", dtype="f64",
                                     group="data"))
                if bufs.gpu:
                    torch.cuda.synchronize()
                red = (flat / size).cpu().numpy()
            off = 0
            for n in b:
                k = tw[n].numel()
                want[n] = red[off:off + k]
                off += k
        model.zero_grad(set_to_none=True)
        model(xs[rank].to(dev)).backward()
        dd.finish_gradients()
        if bufs.gpu:
            torch.cuda.synchronize()
        h = hashlib.sha256()
        for n, p in model.named_parameters():
            got = p.grad.detach().cpu().numpy().reshape(-1)
            if got.dtype == np.float32:
                bad = int((got.view(np.uint32) != want[n].view(np.uint32)).sum())
                assert bad == 0, (it, n, f"{bad} of {got.size} elements differ")
            else:
                assert np.allclose(got, want[n], rtol=0, atol=1e-12), (it, n)
            h.update(got.tobytes())
        print(f"DIGEST {rank} {h.hexdigest()}")
    # a non-contiguous gradient is refused by name
    model.zero_grad(set_to_none=True)
    model.b2.grad = torch.zeros(300, device=dev)
    model.w2.grad = torch.zeros(3, 300, device=dev).t()
    assert not model.w2.grad.is_contiguous()
    ps_w2 = dd._buckets[dd._param_bucket[id(model.w2)]]
    assert [names[id(p)] for p in ps_w2] == ["b2", "w2"]
    _raises(ValueError, "contiguous", lambda: [dd._hook(p) for p in ps_w2])
    dd.close()
    assert all(r is None for r in dd._seg)
    for r in refs:
        if r is not None:
            r.destroy()
    d.barrier("global")
    mx.finalize()


WORKERS = {
    "seg_check": seg_check,
    "seg_env_algo": seg_env_algo,
    "seg_refusals": seg_refusals,
    "seg_plugin": seg_plugin,
    "ddp_check": ddp_check,
}


def main():
    name = sys.argv[1]
    kwargs = json.loads(sys.argv[2]) if len(sys.argv) > 2 else {}
    WORKERS[name](**kwargs)
    print(f"OK {name} rank={os.environ.get('RANK')}")


if __name__ == "__main__":
    main()
