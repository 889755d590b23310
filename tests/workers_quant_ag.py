"""Quantized all-gather: what its tests share, and their rank workers.

Every rank's contribution is quantized once, travels as it is and is decoded
the same way on every rank, the contributor included, so the result is a
fixed function of the inputs at any world size: `ref_segments` over the
reference-quantized contributions, assigned or accumulated. Helpers, shapes
and inputs come from tests/workers_quant_rs.py and tests/quant_ref.py; this
module adds the segmented reference, the kernel cases, a launcher for its own
workers, and the workers (TCP host transport with numpy buffers, or every
rank on GPU 0 with torch buffers or pageable numpy buffers; QRS_DEVICE picks).

Run as: python -m tests.workers_quant_ag <worker> '<json kwargs>'
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

def ref_segments(wire, nseg, count, block, dtype, base=None):
    """Bits of the segmented dequantize of `wire` (nseg segment wires, each
    on a block grid of its own). base=None assigns: qr.ref_dequantize per
    segment. Otherwise `base` (nseg * count elements in `dtype` storage) is
    accumulated into: per element fma(q, scale, base), rounded once to
    float32 and then stored in `dtype`.

    q * scale is exact in float64 (8 x 24 bits). Adding the float32 base to
    it is exact in float64 while every bit of either lies in a window of 53
    binary places; the one rounding to float32 then makes the sum a correctly
    rounded fma. Asserted here: scales in [2^-20, 2^1), so that products are
    multiples of 2^-43 below 2^8, and base values below 2^8 that are
    multiples of 2^-43 as well: 51 places."""
    seg_wire = qr.wire_bytes(count, block)
    out = []
    for j in range(nseg):
        s, _, q = qr.parse_wire(wire[j * seg_wire:(j + 1) * seg_wire], block)
        if base is None:
            out.append(qr.ref_dequantize(s, q, count, dtype).view(BITS[dtype]))
            continue
        b = qr.decode(base[j * count:(j + 1) * count], dtype)
        assert s.min() >= 2.0 ** -20 and s.max() < 2.0, "scales: reference not exact"
        grid = b.astype(F64) * 2.0 ** 43
        assert np.abs(b).max() < 2.0 ** 8 and (grid == np.rint(grid)).all(), \
            "base: reference not exact"
        prod = (q.astype(F64) * s.astype(F64)[:, None]).reshape(-1)[:count]
        out.append(qr.encode((prod + b.astype(F64)).astype(F32), dtype).view(BITS[dtype]))
    return np.concatenate(out)


# nseg of the kernel tests: 9 shows that there is no 8-wire cap
KERNEL_NSEG = [1, 3, 8, 9]
SMALL_CASES = [c for c in w.KERNEL_CASES if c[0] < (1 << 20)]
assert len(SMALL_CASES) == 5
# One pass of the grid is 8192 wire blocks on the generic path and 16384 on
# the fast path (w.KERNEL_CASES). Three segments of 2731 (5463) blocks are
# 8193 (16389) blocks: the second pass starts inside segment 2.
MULTIPASS_CASES = [(2731 * 128 - 5, 128), (5463 * 256, 256)]
MULTIPASS_NSEG = 3

# (count, block, offset_elems of `out`, nseg, accumulate, dtype)
KERNEL_PARAMS = (
    [(c, b, 0, n, acc, dt) for c, b in SMALL_CASES for n in KERNEL_NSEG
     for acc in (False, True) for dt in ("f32", "bf16")] +
    [w.OFFSET_CASE + (1, 3, acc, dt) for acc in (False, True) for dt in ("f32", "bf16")] +
    [(c, b, 0, MULTIPASS_NSEG, True, "f32") for c, b in MULTIPASS_CASES])


@functools.lru_cache(maxsize=None)
def kernel_wire(nseg, count, block):
    """`nseg` segment wires, one after the other, from ref_quantize(randn *
    m) with m spread over [1, 7]. Cached: read-only."""
    rng = np.random.default_rng(count * 16 + nseg)
    muls = np.linspace(1.0, 7.0, nseg) if nseg > 1 else [1.0]
    wire = np.concatenate([
        qr.ref_wire(*qr.ref_quantize((rng.standard_normal(count) * m).astype(F32), block))
        for m in muls])
    wire.setflags(write=False)
    return wire


@functools.lru_cache(maxsize=None)
def kernel_base(nseg, count, dtype):
    """What `out` holds before an accumulate: magnitudes in [0.25, 4) with a
    random sign, in `dtype` storage. Cached: read-only."""
    rng = np.random.default_rng(count * 32 + nseg)
    n = nseg * count
    v = (rng.uniform(0.25, 4.0, n) * rng.choice([-1.0, 1.0], n)).astype(F32)
    base = qr.encode(v, dtype)
    mag = np.abs(qr.decode(base, dtype))
    assert mag.min() >= 0.25 and mag.max() <= 4.0
    base.setflags(write=False)
    return base


@functools.lru_cache(maxsize=None)
def kernel_expectation(nseg, count, block, dtype, accumulate):
    want = ref_segments(kernel_wire(nseg, count, block), nseg, count, block, dtype,
                        kernel_base(nseg, count, dtype) if accumulate else None)
    want.setflags(write=False)
    return want


def host_dequantize_segments(wire, nseg, count, block, dtype, accumulate, offset_elems=0,
                             sentinel=0xCD):
    """ops.host_dequantize_segments into a guarded buffer; returns out's
    bits. Sentinels sit around `out` and behind the wire; the wire is
    compared with its original afterwards. `out` starts as kernel_base when
    accumulating and as 0xAB bytes otherwise."""
    from mlsl_amd import ops
    front = qr.GUARD + offset_elems * ITEM[dtype]
    nbytes = nseg * count * ITEM[dtype]
    whole = np.full(front + nbytes + qr.GUARD, sentinel, dtype=np.uint8)
    whole[front:front + nbytes] = (kernel_base(nseg, count, dtype).view(np.uint8)
                                   if accumulate else 0xAB)
    out = whole[front:front + nbytes].view(NP_DT[dtype])
    g = np.full(wire.size + qr.GUARD, sentinel, dtype=np.uint8)
    g[:wire.size] = wire
    ops.host_dequantize_segments(g[:wire.size], out, count, nseg, block=block, dtype=dtype,
                                 accumulate=accumulate)
    assert np.array_equal(g[:wire.size], wire), "wire modified"
    assert (g[wire.size:] == sentinel).all(), "write behind the wire"
    assert (whole[:front] == sentinel).all() and (whole[front + nbytes:] == sentinel).all(), \
        "write outside out"
    return out.view(BITS[dtype]).copy()


# ---- collective expectations -----------------------------------------------

def gather_wire(size, count, block, dtype):
    """The wire every rank holds after the exchange: the reference-quantized
    w.rank_input of every rank, in rank order."""
    return np.concatenate([
        qr.ref_wire(*qr.ref_quantize(qr.decode(w.rank_input(r, count, dtype), dtype), block))
        for r in range(size)])


def recv_base(n, dtype):
    """recv on entry to an accumulating all-gather: the same on every rank."""
    rng = np.random.default_rng(77)
    v = (rng.uniform(0.25, 4.0, n) * rng.choice([-1.0, 1.0], n)).astype(F32)
    return qr.encode(v, dtype)


# ---- launcher --------------------------------------------------------------

def run_ranks(worker, world, device=False, timeout=120, extra_env=None, **kwargs):
    """tests.workers_quant_ag.<worker>(**kwargs) in `world` processes, on the
    TCP transport or (device=True or "numpy") all on GPU 0. Every process
    gets `timeout` seconds; the first to exceed it takes all ranks down.
    Raises on a nonzero exit; returns the stdouts."""
    port = free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ)
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
            [sys.executable, "-m", "tests.workers_quant_ag", worker, json.dumps(kwargs)],
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


def assert_one_digest(outs, world):
    """Every rank printed the same non-empty list of digests."""
    found = digests(outs)
    assert sorted(found) == list(range(world)), sorted(found)
    assert found[0] and all(found[r] == found[0] for r in found), found


# ---- workers ---------------------------------------------------------------

def ag_check(shapes=None, dtypes=("f32", "bf16"), modes=("assign", "accumulate"),
             inplace=(False, True)):
    """Two starts of one persistent quantized all-gather per configuration.
    After each, recv equals the reference bit for bit on every rank: the
    dequantized contributions in assign mode (the second start gives the same
    bits again: nothing is carried over), the reference applied once and then
    twice in accumulate mode. Out of place the send buffer is left alone; in
    place (assign only) the contribution is this rank's part of recv."""
    mx, bufs, rank, size = w._init()
    d = mx.Distribution(size, 1)
    for dtype in dtypes:
        for count, block in (shapes or w.COLL_SHAPES):
            mx.set_quant_params(block)
            wire = gather_wire(size, count, block, dtype)
            x = w.rank_input(rank, count, dtype)
            for mode in modes:
                acc = mode == "accumulate"
                for ip in inplace:
                    if ip and acc:
                        continue
                    what = (size, dtype, count, block, mode,
                            "inplace" if ip else "outofplace")
                    req = mx.PersistentRequest(d, "all_gather", count, dtype=dtype,
                                               group="data", quantized=True, accumulate=acc)
                    start = recv_base(size * count, dtype)
                    want = start.view(BITS[dtype])
                    recv = bufs.put(start)
                    for k in range(2):
                        if ip:
                            recv[rank * count:(rank + 1) * count] = bufs.put(x)
                            send = recv[rank * count:(rank + 1) * count]
                        else:
                            send = bufs.put(x)
                        req.start(send, recv)
                        req.wait()
                        got = bufs.get(recv, dtype)
                        want = ref_segments(wire, size, count, block, dtype,
                                            want.view(NP_DT[dtype]) if acc else None)
                        bad = int((got.view(BITS[dtype]) != want).sum())
                        assert bad == 0, (what, f"start {k}: {bad} of {size * count} "
                                                "elements differ from the reference")
                        if not ip:
                            assert np.array_equal(bufs.get(send, dtype), x), \
                                (what, "send buffer modified")
                        print(f"DIGEST {rank} {hashlib.sha256(got.tobytes()).hexdigest()}")
                    req.destroy()
    mx.set_quant_params(256)
    d.barrier("global")
    mx.finalize()


def ag_errors():
    """What the interfaces refuse: f64 and a compression plugin with an error
    from the library that names the reason, and the three argument errors of
    PersistentRequest."""
    import ctypes
    from ctypes import byref, c_char_p, c_size_t, c_void_p
    assert os.path.exists(w.PLUGIN), "build the plugin first: ensure_plugin()"
    mx, bufs, rank, size = w._init()
    from mlsl_amd._lib import lib
    L = lib()
    d = mx.Distribution(size, 1)

    def error_of(exc, f):
        try:
            f()
        except exc as e:
            return str(e)
        raise AssertionError(f"no {exc.__name__}")

    for acc in (False, True):
        msg = error_of(RuntimeError, lambda: mx.PersistentRequest(
            d, "all_gather", 64, dtype="f64", group="data", quantized=True, accumulate=acc))
        assert "f32/bf16" in msg, msg
    error_of(ValueError, lambda: mx.PersistentRequest(
        d, "all_gather", 64, dtype="f32", group="data", accumulate=True))
    error_of(ValueError, lambda: mx.PersistentRequest(
        d, "all_reduce", 64, dtype="f32", group="data", quantized=True, accumulate=True))
    error_of(ValueError, lambda: mx.PersistentRequest(
        d, "all_to_all", 64, dtype="f32", group="data", quantized=True))
    # the exact requests still build
    mx.PersistentRequest(d, "all_gather", 64, dtype="f64", group="data").destroy()
    mx.PersistentRequest(d, "all_to_all", 64, dtype="f32", group="data").destroy()

    class QP(ctypes.Structure):
        _fields_ = [("lib_path", c_char_p), ("quant", c_char_p),
                    ("dequant", c_char_p), ("reduce_sum", c_char_p),
                    ("block_size", c_size_t), ("elem_in_block", c_size_t)]

    env = c_void_p()
    assert L.mlsl_environment_get_env(byref(env)) == 0
    assert L.mlsl_environment_set_quantization_params(
        env, byref(QP(w.PLUGIN.encode(), None, None, None, 264, 256))) == 0, \
        ctypes.string_at(L.mlsl_last_error()).decode()
    msg = error_of(RuntimeError, lambda: mx.PersistentRequest(
        d, "all_gather", 1003, dtype="f32", group="data", quantized=True))
    assert "plugin" in msg, msg
    L.mlsl_environment_set_quantization_params(
        env, byref(QP(None, None, None, None, 0, 256)))
    d.barrier("global")
    mx.finalize()


def _identical_across_ranks(mx, d, torch, flat, gpu, what):
    for op in ("min", "max"):
        red = torch.empty_like(flat)
        mx.wait(d.all_reduce(flat, red, flat.numel(), op=op, group="data"))
        if gpu:
            torch.cuda.synchronize()
        assert torch.equal(red, flat), f"{what}: parameters differ across ranks"


def ag_sharded_optimizer(compression="none", rs_algo=None):
    """ShardedOptimizer(ag_compression="int8") on f32 parameters, SGD, one
    quantization block of 128 per shard of 106: a normal step, then a step
    with zero gradients.

    After every step `flat` is identical across ranks, and against the exact
    master shards (gathered exactly) every element obeys

        |flat - master| <= m/254 * (1 + 2^-14) + 2^-24 |d| + 2^-24 |flat|

    where d = master - flat_before is this step's delta and m the largest
    |d| of the element's block. From the arithmetic: the delta sent is
    fl(d), off by at most half an ulp, 2^-24 |d|. The codec takes scale =
    fl(m/127) <= m/127 (1 + 2^-24) and q = rint(fl(fl(d) * fl(1/scale))); the
    two roundings move the quotient, at most 127 in magnitude, by less than
    127 * 2.1 * 2^-24 < 2^-16, so |q - fl(d)/scale| <= 1/2 + 2^-16 and
    |q * scale - fl(d)| <= m/254 * (1 + 2^-24)(1 + 2^-15) < m/254 * (1 +
    2^-14). flat = fl(fma(q, scale, flat_before)) adds half an ulp of the
    result, 2^-24 |flat|.

    The second step's gradients are zero, so master stays and the delta is
    the first step's error e1 <= m1/254: the new error is at most
    e1/254 (1 + 2^-14) plus the same roundings, asserted as e1/100 plus one
    ulp of the largest parameter."""
    mx, bufs, rank, size = w._init()
    import torch
    from mlsl_amd.parallel.zero1 import ShardedOptimizer
    dev = "cuda" if bufs.gpu else "cpu"
    d = mx.Distribution(size, 1)
    block = 128
    mx.set_quant_params(block)

    try:
        ShardedOptimizer([torch.nn.Parameter(torch.zeros(8, dtype=torch.float64))],
                         torch.optim.SGD, d, ag_compression="int8", lr=0.1)
    except ValueError as e:
        assert "f32/bf16" in str(e), str(e)
    else:
        raise AssertionError('ag_compression="int8" accepted f64 parameters')

    torch.manual_seed(7)
    model = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Tanh(),
                                torch.nn.Linear(16, 4)).to(dev)   # 212 parameters
    opt = ShardedOptimizer(model.parameters(), torch.optim.SGD, d, reduce="rs",
                           compression=compression, rs_algo=rs_algo,
                           ag_compression="int8", lr=0.1)
    assert opt.master is not None and opt.shard == 106
    g = torch.Generator().manual_seed(100 + rank)
    xb = torch.randn(32, 8, generator=g).to(dev)
    yb = torch.randn(32, 4, generator=g).to(dev)
    errs = []
    for step in range(2):
        before = opt.flat.detach().clone()
        opt.zero_grad()
        if step == 0:
            torch.nn.functional.mse_loss(model(xb), yb).backward()
        else:
            for p in opt.params:
                p.grad = torch.zeros_like(p)
        opt.step()
        flat = opt.flat.detach()
        _identical_across_ranks(mx, d, torch, flat, bufs.gpu, f"step {step}")
        master = torch.empty_like(flat)
        mx.wait(d.all_gather(opt.master, opt.shard, master, dtype="f32", group="data"))
        if bufs.gpu:
            torch.cuda.synchronize()
        m64 = master.double().cpu().numpy()
        f64 = flat.double().cpu().numpy()
        delta = m64 - before.double().cpu().numpy()
        err = np.abs(f64 - m64)
        bound = np.empty_like(err)
        for r in range(size):
            for lo in range(r * opt.shard, (r + 1) * opt.shard, block):
                hi = min(lo + block, (r + 1) * opt.shard)
                bound[lo:hi] = np.abs(delta[lo:hi]).max() / 254 * (1 + 2.0 ** -14)
        bound += 2.0 ** -24 * np.abs(delta) + 2.0 ** -24 * np.abs(f64)
        print(f"step {step}: max error {err.max():.3e}, max bound {bound.max():.3e}, "
              f"max |delta| {np.abs(delta).max():.3e}")
        assert (err <= bound).all(), (step, float((err - bound).max()))
        errs.append(float(err.max()))
        if step == 0:
            assert np.abs(delta).max() > 0 and err.max() > 0, "nothing was quantized"
    ulp = float(np.spacing(np.abs(f64).max().astype(F32)))
    print(f"max error after the step {errs[0]:.3e}, after the zero-gradient step "
          f"{errs[1]:.3e} (allowed {errs[0] / 100 + ulp:.3e})")
    if compression == "none":
        # (a compressed reduce_scatter flushes its residual into the second
        # step's gradients: master moves, and the delta is more than e1)
        assert errs[1] <= errs[0] / 100 + ulp, errs
    mx.set_quant_params(256)
    d.barrier("global")
    mx.finalize()


WORKERS = {
    "ag_check": ag_check,
    "ag_errors": ag_errors,
    "ag_sharded_optimizer": ag_sharded_optimizer,
}


def main():
    name = sys.argv[1]
    kwargs = json.loads(sys.argv[2]) if len(sys.argv) > 2 else {}
    WORKERS[name](**kwargs)
    print(f"OK {name} rank={os.environ.get('RANK')}")


if __name__ == "__main__":
    main()
