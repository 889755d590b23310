"""The exact allreduce over a list of tensors: the kernel case its CPU and GPU
tests share (numpy on the concatenation, tests/quant_seg_ref.py's arenas), and
the rank workers (python -m tests.workers_list_exact <worker> '<json kwargs>')."""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

from tests import quant_seg_ref as sr
from tests import workers_quant_rs as w
from tests import workers_quant_seg as ws
from tests.mp import REPO, free_port

F32, qr = np.float32, sr.qr
ITEM = {"f32": 4, "bf16": 2, "f16": 2}
BITS = {"f32": np.uint32, "bf16": np.uint16, "f16": np.uint16}
LAYOUTS = ("one", "edges", "tiny700", "fastslow")
# bases 0, 1 and 2 elements past a 16-byte boundary reach the 16-byte, dword and
# halfword regimes of a 2-byte type and both of f32; "trip" passes one launch
PARAMS = [(lay, dt, shift) for lay in LAYOUTS for dt in ITEM for shift in (0, 1, 2)] + \
         [("trip", dt, 1) for dt in ITEM]
PS3 = sr.POST_SCALES[2]   # 1/3


def counts_of(layout, dtype):
    if layout != "trip":
        return sr.LAYOUTS[layout]
    from mlsl_amd import ops   # the second trip starts 500 elements before tensor 1 ends
    return [1000, ops.list_elems_per_trip(dtype) - 500, 3000]


def decode(bits, dtype):
    return bits.view(np.float16).astype(F32) if dtype == "f16" \
        else qr.decode(bits.view(sr.NP_DT[dtype]), dtype)


def encode(x, dtype):
    """float32 -> `dtype` bits, round to nearest even."""
    return x.astype(np.float16).view(np.uint16) if dtype == "f16" \
        else qr.encode(x, dtype).view(BITS[dtype])


@functools.lru_cache(maxsize=None)
def case_input(count, dtype):
    """`count` bit patterns, read-only: the helpers' randn * 3 with a NaN that
    carries a payload, a -0 and the subnormal 3 planted: 3 * 0.5 is a rounding
    tie in every dtype (even: 2). Under float32(1/3) no bf16 or f16 value is a
    tie: the product's dropped bits stay 1/6 of a unit away from the half."""
    v = encode(qr.decode(ws.start_input(0, 0, count, "f32"), "f32"), dtype).copy()
    v[count // 2] = {"f32": 0x7FC00015, "bf16": 0x7FC5, "f16": 0x7E15}[dtype]
    v[count // 3] = 1 << (8 * ITEM[dtype] - 1)
    v[count - 1] = 3
    v.setflags(write=False)
    return v


def arena_of(counts, dtype, shift):
    """sr.Arena with every base `shift` elements past a 16-byte boundary."""
    a = sr.Arena(counts, "f32" if dtype == "f32" else "bf16", False)
    a.starts = [s + shift * a.item for s in a.starts]
    a.guard[:] = True
    for s, n in zip(a.starts, counts):
        a.guard[s:s + n * a.item] = False
    return a


def run_list_case(api, kind, layout, dtype, shift):
    """ops.<kind>gather_list, then ops.<kind>scatter_scale_list at post_scale 1, 0.5 and 1/3, against numpy
    on the concatenation, bit for bit (a NaN for a NaN where the product ran);
    sentinels around `flat` and every tensor intact, inputs unchanged."""
    from mlsl_amd import ops
    gather, scatter = getattr(ops, kind + "gather_list"), getattr(ops, kind + "scatter_scale_list")
    counts = counts_of(layout, dtype)
    count, item = sum(counts), ITEM[dtype]
    nbytes, v = count * item, case_input(sum(counts), dtype)
    arena = arena_of(counts, dtype, shift)
    tensors = lambda buf: [buf[s:s + n * item] for s, n in zip(arena.starts, counts)]  # noqa: E731

    in_img = arena.fill(v)
    d_in = api.put(in_img)
    flat_img, lo = sr.guarded_bytes(nbytes, 0xAB)
    d_flat = api.put(flat_img)
    gather(tensors(d_in), counts, d_flat[lo:lo + nbytes], dtype=dtype)
    h_flat = api.get(d_flat)
    assert np.array_equal(api.get(d_in), in_img), "the gather wrote to a tensor"
    assert sr.body_intact(h_flat, nbytes), "the gather wrote outside flat[0, count)"
    assert np.array_equal(h_flat[lo:lo + nbytes].view(BITS[dtype]), v), "gather"

    outs = {}
    for ps in sr.POST_SCALES:
        d_out = api.put(arena.blank())
        scatter(d_flat[lo:lo + nbytes], tensors(d_out), counts, dtype=dtype, post_scale=ps)
        h_out = api.get(d_out)
        assert arena.guards_intact(h_out), "write outside the tensors"
        got = arena.gather(h_out).view(BITS[dtype])
        ref = v if ps == 1.0 else encode((decode(v, dtype) * F32(ps)).astype(F32), dtype)
        nan = np.isnan(decode(ref, dtype)) & (ps != 1.0)
        assert np.isnan(decode(got, dtype))[nan].all(), "NaN"
        bad = np.flatnonzero((got != ref) & ~nan)
        assert bad.size == 0, (ps, bad.size, bad[:4], got[bad[:4]], ref[bad[:4]], v[bad[:4]])
        outs[ps] = np.where(nan, 0, got)
    assert np.array_equal(api.get(d_flat), h_flat), "the scatter wrote to flat"
    return outs


def run_ranks(worker, world, device=False, extra_env=None, **kwargs):
    """ws.run_ranks for this module's workers; the ranks' digests must agree."""
    port, procs = free_port(), []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MLSL_PORT=str(port), PYTHONPATH=REPO, QRS_DEVICE=w.qrs_device(device),
                   **(extra_env or {}))
        env.pop("MLSL_TRANSPORT", None)
        env.update({"MLSL_TIMEOUT": "90"} if device else {"MLSL_TRANSPORT": "tcp"})
        procs.append(subprocess.Popen(
            [sys.executable, "-m", "tests.workers_list_exact", worker, json.dumps(kwargs)],
            env=env, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    try:
        outs = [p.communicate(timeout=120)[0] for p in procs]
    finally:
        for p in procs:
            p.kill()
    failed = [f"--- rank {r} rc={p.returncode} ---\n{o[-3000:]}"
              for r, (p, o) in enumerate(zip(procs, outs)) if p.returncode != 0]
    assert not failed, f"{worker} world={world} failed:\n" + "\n".join(failed)
    ws.assert_ranks_agree(outs, world)


def list_check():
    """SegmentedAllReduce(compression=None, post_scale=1/3) against the flat
    exact all_reduce of the concatenation times float32(1/3): three starts,
    fresh tensors each. Integer inputs in [-16, 16] keep every partial sum
    exact, so the flat reference is one value whatever order it sums in (its
    small-message schedule from three ranks on reduces in arrival order)."""
    mx, bufs, rank, size = w._init()
    d = mx.Distribution(size, 1)
    for counts in sr.COLL_LAYOUTS.values():
        count, offs = sum(counts), sr.offsets(counts)
        for dtype in ("f32", "bf16"):
            req = mx.SegmentedAllReduce(d, counts, dtype=dtype, group="data", post_scale=PS3,
                                        compression=None)
            keep, h = [], hashlib.sha256()
            for s in range(ws.STARTS):
                rng = np.random.default_rng(7000 + 97 * rank + s)
                x = encode(rng.integers(-16, 17, count).astype(F32), dtype).view(sr.NP_DT[dtype])
                flat = bufs.put(x)
                mx.wait(d.all_reduce(flat, flat, count, op="sum", dtype=dtype, group="data"))
                want = encode((decode(bufs.get(flat, dtype), dtype) * F32(PS3)).astype(F32),
                              dtype)
                keep.append([bufs.put(x[offs[j]:offs[j + 1]]) for j in range(len(counts))])
                req.start(keep[-1])
                req.wait()
                got = np.concatenate([bufs.get(t, dtype) for t in keep[-1]]).view(BITS[dtype])
                assert np.array_equal(got, want), (size, dtype, count, s, int((got != want).sum()))
                h.update(got.tobytes())
            print(f"DIGEST {rank} {h.hexdigest()}")
            req.destroy()
    d.barrier("global")
    mx.finalize()


def list_refusals():
    """Refusals by message; a refused start leaves the request usable."""
    mx, bufs, rank, size = w._init()
    d = mx.Distribution(size, 1)
    mk = lambda counts, **kw: lambda: mx.SegmentedAllReduce(  # noqa: E731
        d, counts, group="data", **{"compression": None, **kw})
    ws._raises(ValueError, "it needs compression='int8' or 'int4'", mk([4], ar_algo="ring"))
    ws._raises(RuntimeError, "supports f32/bf16/f16 only", mk([4, 4], dtype="f64"))
    ws._raises(RuntimeError, "nseg == 0", mk([]))
    ws._raises(RuntimeError, "tensor 1 has a zero count", mk([4, 0, 4]))
    req = mk([3, 5], dtype="f16", post_scale=0.5)()
    a, b = (bufs.put(np.ones(n, np.float16).view(np.uint16)) for n in (3, 5))
    ws._raises(RuntimeError, "nseg differs from creation", lambda: req.start([a]))
    ws._raises(RuntimeError, "tensor 1 is null", lambda: req.start([a, 0]))
    if bufs.gpu:
        ws._raises(RuntimeError, "tensor 1 is not device memory",
                   lambda: req.start([a, np.ones(5, np.float16)]))
    from mlsl_amd._lib import lib
    assert lib().mlsl_request_start(req._h, None, None) != 0, "the flat start is not its own"
    if size == 1 or bufs.gpu:   # the host transport has no f16 sum
        req.start([a, b])
        req.wait()
        for t in (a, b):
            assert (bufs.get(t, "bf16").view(np.float16) == 0.5 * size).all()
    req.destroy()
    print(f"DIGEST {rank} refused")
    d.barrier("global")
    mx.finalize()


def ddp_check(with_f64=False):
    """DistributedData(grads="in_place") against one flat exact all_reduce per
    f32 bucket on torch.cat of a twin model's gradients, times float32(1 /
    world); an f64 bucket stays on the cat path. Ranks compare values at world
    2 only: from three on the flat schedule's order depends on the rank."""
    mx, bufs, rank, size = w._init()
    import torch
    from mlsl_amd.parallel import DistributedData
    dev = "cuda" if bufs.gpu else "cpu"
    torch.manual_seed(11)
    model, twin = ws._mlp(torch, with_f64).to(dev), ws._mlp(torch, with_f64).to(dev)
    d = mx.Distribution(size, 1)
    dd = DistributedData(model, dist=d, bucket_mb=0.003, grads="in_place")
    twin.load_state_dict(model.state_dict())
    tw = {id(p): q for p, q in zip(model.parameters(), twin.parameters())}
    assert sum(s is not None for s in dd._seg) == 2 and len(dd._seg) == 2 + with_f64
    for it in range(3):
        x = torch.randn(6, 5, generator=torch.Generator().manual_seed(300 + it * size + rank))
        twin.zero_grad(set_to_none=True)
        twin(x.to(dev)).backward()
        model.zero_grad(set_to_none=True)
        model(x.to(dev)).backward()
        dd.finish_gradients()
        h = hashlib.sha256()
        for ps, seg in zip(dd._buckets, dd._seg):
            flat = torch.cat([tw[id(p)].grad.detach().reshape(-1) for p in ps])
            mx.wait(d.all_reduce(flat, flat, flat.numel(), op="sum",
                                 dtype="f32" if seg is not None else "f64", group="data"))
            if bufs.gpu:
                torch.cuda.synchronize()
            want = (flat.cpu().numpy() * F32(1.0 / size)).astype(F32) if seg is not None \
                else (flat / size).cpu().numpy()
            got = torch.cat([p.grad.detach().reshape(-1) for p in ps]).cpu().numpy()
            assert np.array_equal(got, want), (it, got.dtype, int((got != want).sum()))
            h.update(got.tobytes() if size == 2 else b"matched")
        print(f"DIGEST {rank} {h.hexdigest()}")
    dd.close()
    assert all(s is None for s in dd._seg)
    d.barrier("global")
    mx.finalize()


if __name__ == "__main__":
    {f.__name__: f for f in (list_check, list_refusals, ddp_check)}[sys.argv[1]](
        **(json.loads(sys.argv[2]) if len(sys.argv) > 2 else {}))
    print(f"OK {sys.argv[1]} rank={os.environ.get('RANK')}")
