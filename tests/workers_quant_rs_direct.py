"""One-shot (direct) quantized reduce-scatter: what its tests share, and
their rank workers.

The direct algorithm quantizes every contribution once and sums the N wires
of a segment in rank order with one fma per wire, so its result is a fixed
function of the inputs at any world size: `ref_sum_dequant_n` over the
reference-quantized segments. Helpers, shapes and inputs come from
tests/workers_quant_rs.py and tests/quant_ref.py; this module adds the N-way
reference, the kernel cases, a launcher for its own workers, and the workers
(TCP host transport with numpy buffers, or every rank on GPU 0 with torch
buffers; QRS_DEVICE picks).

Run as: python -m tests.workers_quant_rs_direct <worker> '<json kwargs>'
"""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

from tests import quant_ref as qr
from tests import workers_quant_rs as w
from tests.mp import REPO, free_port

F32, F64 = np.float32, np.float64
ITEM, NP_DT, BITS = w.ITEM, w.NP_DT, w.BITS


# ---- expectations ----------------------------------------------------------

def ref_sum_dequant_n(wires, count, block, dtype):
    """Bits of the N-way sum-dequantize: per element acc = +0, then per wire
    in order acc = fma(q, scale, acc), stored in `dtype`.

    q * scale is exact in float64 (8 x 24 bits), and adding a float32 to it
    is exact in float64 while the two are within 2^20 of each other, so the
    one rounding to float32 makes this a correctly rounded fma. Block scales
    of wires that differ by less than 2^16 keep it so; asserted here."""
    parsed = [qr.parse_wire(x, block) for x in wires]
    scales = np.stack([p[0] for p in parsed]).astype(F64)
    ratio = float((scales.max(axis=0) / scales.min(axis=0)).max())
    assert ratio < 2.0 ** 16, f"scale ratio {ratio} across wires: reference not exact"
    acc = np.zeros(parsed[0][2].shape, dtype=F32)
    for s, _, q in parsed:
        acc = (q.astype(F64) * s.astype(F64)[:, None] + acc.astype(F64)).astype(F32)
    return qr.encode(acc.reshape(-1)[:count], dtype).view(BITS[dtype])


# nwires of the kernel tests, and the (count, block) cases of
# w.KERNEL_CASES split by cost: the two multi-pass shapes (a second trip
# round the grid-stride loop) run at one nwires and f32 only
KERNEL_NWIRES = [1, 2, 3, 8]
SMALL_CASES = [c for c in w.KERNEL_CASES if c[0] < (1 << 20)]
MULTIPASS_CASES = [c for c in w.KERNEL_CASES if c[0] >= (1 << 20)]
MULTIPASS_NWIRES = 3
assert len(SMALL_CASES) == 5 and len(MULTIPASS_CASES) == 2

# (count, block, offset_elems of `out`, nwires, dtype)
KERNEL_PARAMS = (
    [(c, b, 0, n, dt) for c, b in SMALL_CASES for n in KERNEL_NWIRES
     for dt in ("f32", "bf16")] +
    [w.OFFSET_CASE + (1, n, dt) for n in KERNEL_NWIRES for dt in ("f32", "bf16")] +
    [(c, b, 0, MULTIPASS_NWIRES, "f32") for c, b in MULTIPASS_CASES])


@functools.lru_cache(maxsize=None)
def kernel_wires(nwires, count, block):
    """`nwires` wires from ref_quantize(randn * m), m spread over [1, 7], so
    that block scales differ (by a factor of about 7 at the most). Cached:
    treat as read-only."""
    rng = np.random.default_rng(count * 16 + nwires)
    muls = np.linspace(1.0, 7.0, nwires) if nwires > 1 else [1.0]
    out = []
    for m in muls:
        wire = qr.ref_wire(*qr.ref_quantize((rng.standard_normal(count) * m).astype(F32),
                                            block))
        wire.setflags(write=False)
        out.append(wire)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def kernel_expectation(nwires, count, block, dtype):
    want = ref_sum_dequant_n(kernel_wires(nwires, count, block), count, block, dtype)
    want.setflags(write=False)
    return want


def host_sum_dequant_n(wires, count, block, dtype, offset_elems=0, sentinel=0xCD):
    """ops.host_quant_sum_dequant_n into a guarded buffer; returns out's
    bits. Sentinels sit around `out` and behind every wire; the wires are
    compared with their originals afterwards."""
    from mlsl_amd import ops
    front = qr.GUARD + offset_elems * ITEM[dtype]
    nbytes = count * ITEM[dtype]
    whole = np.full(front + nbytes + qr.GUARD, sentinel, dtype=np.uint8)
    whole[front:front + nbytes] = 0xAB
    out = whole[front:front + nbytes].view(NP_DT[dtype])
    guarded = []
    for x in wires:
        g = np.full(x.size + qr.GUARD, sentinel, dtype=np.uint8)
        g[:x.size] = x
        guarded.append(g)
    ops.host_quant_sum_dequant_n([g[:x.size] for g, x in zip(guarded, wires)], out, count,
                                 block=block, dtype=dtype)
    for g, x in zip(guarded, wires):
        assert np.array_equal(g[:x.size], x), "wire modified"
        assert (g[x.size:] == sentinel).all(), "write behind a wire"
    assert (whole[:front] == sentinel).all() and (whole[front + nbytes:] == sentinel).all(), \
        "write outside out"
    return out.view(BITS[dtype]).copy()


def expected_segment(rank, size, count, block, dtype):
    """Bits of rank `rank`'s output of a direct reduce-scatter's first start
    (zero residual) on w.rank_input: the N-way sum, in rank order, of the
    reference-quantized segment `rank` of every rank's input."""
    segs = [qr.decode(w.rank_input(k, size * count, dtype), dtype)
            [rank * count:(rank + 1) * count] for k in range(size)]
    wires = [qr.ref_wire(*qr.ref_quantize(s, block)) for s in segs]
    return ref_sum_dequant_n(wires, count, block, dtype)


def exact_segment(rank, size, count, dtype):
    return np.sum([qr.decode(w.rank_input(k, size * count, dtype), dtype)
                   [rank * count:(rank + 1) * count].astype(F64) for k in range(size)],
                  axis=0)


# ---- launcher --------------------------------------------------------------

def run_ranks(worker, world, device=False, timeout=120, extra_env=None, **kwargs):
    """tests.workers_quant_rs_direct.<worker>(**kwargs) in `world` processes,
    on the TCP transport or (device=True or "numpy") all on GPU 0. Every process gets
    `timeout` seconds; the first to exceed it takes all ranks down. Raises on
    a nonzero exit; returns the stdouts."""
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
            [sys.executable, "-m", "tests.workers_quant_rs_direct", worker,
             json.dumps(kwargs)],
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


def digests(outs):
    """{rank: [digest, ...]} from the DIGEST lines the workers print."""
    found = {}
    for out in outs:
        for line in out.splitlines():
            if line.startswith("DIGEST "):
                _, rank, dig = line.split()
                found.setdefault(int(rank), []).append(dig)
    return found


# ---- workers ---------------------------------------------------------------

def _reduce_scatter(mx, bufs, d, rank, size, dtype, count, inplace, algo, starts=1):
    """`starts` runs of one persistent quantized reduce-scatter with `algo`
    on this rank's input; returns the outputs and checks that an
    out-of-place run leaves the send buffer alone."""
    x = w.rank_input(rank, size * count, dtype)
    req = mx.PersistentRequest(d, "reduce_scatter", count, dtype=dtype, op="sum",
                               group="data", quantized=True, algo=algo)
    outs = []
    for _ in range(starts):
        send = bufs.put(x)
        recv = (send[rank * count:(rank + 1) * count] if inplace
                else bufs.put(np.zeros(count, dtype=NP_DT[dtype])))
        req.start(send, recv)
        req.wait()
        outs.append(bufs.get(recv, dtype))
        if not inplace:
            assert np.array_equal(bufs.get(send, dtype), x), "send buffer modified"
    req.destroy()
    return outs


def direct_check(shapes=None, dtypes=("f32", "bf16"), algo="direct", compare_ring=True,
                 inplace=(False, True)):
    """The first start of a direct request equals `expected_segment` bit for
    bit on every rank (world 1: dequantize(quantize(x))). From world 3 up
    the ring, on the same inputs, is further from the float64 sum: it
    requantizes the partial sum N-2 times. `algo=None` relies on
    MLSL_QUANT_RS_ALGO=direct in the environment."""
    mx, bufs, rank, size = w._init()
    d = mx.Distribution(size, 1)
    for dtype, count, block, inplace in w._configs(shapes or w.COLL_SHAPES, dtypes,
                                                   inplace):
        mx.set_quant_params(block)
        out = _reduce_scatter(mx, bufs, d, rank, size, dtype, count, inplace, algo)[0]
        what = (size, dtype, count, block, "inplace" if inplace else "outofplace")
        if size == 1:
            seg = qr.decode(w.rank_input(0, count, dtype), dtype)
            want = qr.ref_dequantize(*qr.ref_quantize(seg, block), count, dtype)
            want = want.view(BITS[dtype])
        else:
            want = expected_segment(rank, size, count, block, dtype)
        bad = int((out.view(BITS[dtype]) != want).sum())
        assert bad == 0, (what, f"{bad} of {count} elements differ from the reference")
        if size >= 3 and compare_ring:
            ring = _reduce_scatter(mx, bufs, d, rank, size, dtype, count, inplace, "ring")[0]
            exact = exact_segment(rank, size, count, dtype)
            e_direct = w.rel_l2(qr.decode(out, dtype).astype(F64), exact)
            e_ring = w.rel_l2(qr.decode(ring, dtype).astype(F64), exact)
            print(f"rel_l2 {what}: direct {e_direct:.5f} ring {e_ring:.5f} "
                  f"ratio {e_ring / e_direct:.3f}")
            assert e_direct < e_ring, (what, e_direct, e_ring)
    d.barrier("global")
    mx.finalize()


def direct_error_feedback():
    """Eight starts of one direct request on the same input: the residual
    makes the mean of the outputs converge on the exact sum."""
    mx, bufs, rank, size = w._init()
    d = mx.Distribution(size, 1)
    for count, block in w.COLL_SHAPES:
        mx.set_quant_params(block)
        outs = _reduce_scatter(mx, bufs, d, rank, size, "f32", count, False, "direct",
                               starts=8)
        exact = exact_segment(rank, size, count, "f32")
        first = w.rel_l2(outs[0].astype(F64), exact)
        mean = w.rel_l2(np.mean([o.astype(F64) for o in outs], axis=0), exact)
        print(f"error feedback ({count}, {block}): first {first:.5f} mean of 8 {mean:.5f}")
        assert mean < first / 4, (count, block, first, mean)
    d.barrier("global")
    mx.finalize()


def digest_outputs(algo=None):
    """Print a digest of every configuration's first-start output, for tests
    that compare two launches (with and without MLSL_QUANT_RS_ALGO)."""
    mx, bufs, rank, size = w._init()
    d = mx.Distribution(size, 1)
    for dtype, count, block, inplace in w._configs(w.COLL_SHAPES):
        mx.set_quant_params(block)
        out = _reduce_scatter(mx, bufs, d, rank, size, dtype, count, inplace, algo)[0]
        print(f"DIGEST {rank} {hashlib.sha256(out.tobytes()).hexdigest()}")
    d.barrier("global")
    mx.finalize()


def direct_too_large():
    """More than 8 ranks: the request fails at creation and names the limit;
    the ring still builds."""
    mx, bufs, rank, size = w._init()
    assert size > 8
    d = mx.Distribution(size, 1)
    try:
        mx.PersistentRequest(d, "reduce_scatter", 256, dtype="f32", op="sum",
                             group="data", quantized=True, algo="direct")
    except RuntimeError as e:
        assert "at most 8 ranks" in str(e), str(e)
    else:
        raise AssertionError("direct request on 9 ranks was created")
    mx.PersistentRequest(d, "reduce_scatter", 256, dtype="f32", op="sum",
                         group="data", quantized=True, algo="ring").destroy()
    d.barrier("global")
    mx.finalize()


def direct_plugin():
    """With a compression plugin the direct request fails at creation: the
    plugin ABI has no N-way sum."""
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
    try:
        mx.PersistentRequest(d, "reduce_scatter", 1003, dtype="f32", op="sum",
                             group="data", quantized=True, algo="direct")
    except RuntimeError as e:
        assert "plugin" in str(e), str(e)
    else:
        raise AssertionError("direct request with a compression plugin was created")
    L.mlsl_environment_set_quantization_params(
        env, byref(QP(None, None, None, None, 0, 256)))
    d.barrier("global")
    mx.finalize()


def api_errors():
    """Arguments that name an algorithm where there is none to name."""
    mx, bufs, rank, size = w._init()
    import torch
    from mlsl_amd.parallel.zero1 import ShardedOptimizer
    d = mx.Distribution(size, 1)

    def raises_value_error(f):
        try:
            f()
        except ValueError:
            return True
        return False

    assert raises_value_error(lambda: mx.PersistentRequest(
        d, "reduce_scatter", 64, dtype="f32", op="sum", group="data", algo="direct"))
    assert raises_value_error(lambda: mx.PersistentRequest(
        d, "all_reduce", 64, dtype="f32", op="sum", group="data", quantized=True,
        algo="direct"))
    assert raises_value_error(lambda: mx.PersistentRequest(
        d, "reduce_scatter", 64, dtype="f32", op="sum", group="data", quantized=True,
        algo="tree"))
    params = [torch.nn.Parameter(torch.zeros(8))]
    assert raises_value_error(lambda: ShardedOptimizer(
        params, torch.optim.SGD, d, reduce="rs", rs_algo="direct", lr=0.1))
    assert raises_value_error(lambda: ShardedOptimizer(
        params, torch.optim.SGD, d, reduce="rs", compression="int8", rs_algo="tree",
        lr=0.1))
    d.barrier("global")
    mx.finalize()


def direct_sharded_optimizer():
    """ShardedOptimizer(reduce="rs") uncompressed and with int8 over the
    direct algorithm, from the same start: parameters stay identical across
    ranks, and the compressed step is the exact one up to the quantization
    error."""
    mx, bufs, rank, size = w._init()
    import torch
    from mlsl_amd.parallel.zero1 import ShardedOptimizer
    dev = "cuda" if bufs.gpu else "cpu"
    d = mx.Distribution(size, 1)
    mx.set_quant_params(128)
    steps = {}
    for compression, rs_algo in (("none", None), ("int8", "direct")):
        torch.manual_seed(7)
        model = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Tanh(),
                                    torch.nn.Linear(16, 4)).to(dev)   # 212 parameters
        opt = ShardedOptimizer(model.parameters(), torch.optim.SGD, d, reduce="rs",
                               compression=compression, rs_algo=rs_algo, lr=0.1)
        before = opt.flat.detach().clone()
        g = torch.Generator().manual_seed(100 + rank)
        xb = torch.randn(32, 8, generator=g).to(dev)
        yb = torch.randn(32, 4, generator=g).to(dev)
        torch.nn.functional.mse_loss(model(xb), yb).backward()
        opt.step()
        flat = opt.flat.detach()
        for op in ("min", "max"):
            red = torch.empty_like(flat)
            mx.wait(d.all_reduce(flat, red, flat.numel(), op=op, group="data"))
            if bufs.gpu:
                torch.cuda.synchronize()
            assert torch.equal(red, flat), f"{compression}: parameters differ across ranks"
        steps[compression] = (flat - before).double().cpu().numpy()
    assert np.linalg.norm(steps["none"]) > 0
    rel = w.rel_l2(steps["int8"], steps["none"])
    print(f"sharded optimizer step, int8 direct against none: rel_l2 {rel:.5f}")
    assert 0 < rel < 0.05, rel
    mx.set_quant_params(256)
    d.barrier("global")
    mx.finalize()


WORKERS = {
    "direct_check": direct_check,
    "direct_error_feedback": direct_error_feedback,
    "digest_outputs": digest_outputs,
    "direct_too_large": direct_too_large,
    "direct_plugin": direct_plugin,
    "api_errors": api_errors,
    "direct_sharded_optimizer": direct_sharded_optimizer,
}


def main():
    name = sys.argv[1]
    kwargs = json.loads(sys.argv[2]) if len(sys.argv) > 2 else {}
    WORKERS[name](**kwargs)
    print(f"OK {name} rank={os.environ.get('RANK')}")


if __name__ == "__main__":
    main()
