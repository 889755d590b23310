"""Quantized reduce-scatter: what its tests share, and their rank workers.

Three parts: the expectations of the fused sum-dequantize (the only
arithmetic of a world-2 quantized reduce-scatter after the quantization
itself), a launcher of the shape of tests/mp.py for this module's workers,
and the workers. The workers run unchanged on the TCP host transport (numpy
buffers) and on the device transport with every rank on GPU 0 (torch
buffers, or pageable numpy buffers that the engine stages); QRS_DEVICE picks.

Run as: python -m tests.workers_quant_rs <worker> '<json kwargs>'
"""
import json
import os
import subprocess
import sys

import numpy as np

from tests import quant_ref as qr
from tests.mp import REPO, free_port

F32, F64 = np.float32, np.float64
ITEM = {"f32": 4, "bf16": 2}
NP_DT = {"f32": np.float32, "bf16": np.uint16}
BITS = {"f32": np.uint32, "bf16": np.uint16}

# (count, block) of the kernel tests, device and host alike
KERNEL_CASES = [
    (20, 8),            # generic: fewer elements per block than lanes
    (1003, 128),        # generic: tail block of 107 with a scalar tail of 3
    (1000, 256),        # generic: partial last block, nothing past element 999
    (5000, 512),        # generic: two vector passes per lane
    (1280, 256),        # fast path, 5 blocks: the last pair's second half idles
    # fast path: 2048 workgroups x 4 waves x 2 blocks = 16384 blocks per pass
    (16387 * 256, 256),
    # generic: 2048 workgroups x 4 waves = 8192 blocks per pass
    (8195 * 128, 128),
]
OFFSET_CASE = (1280, 256)   # with `out` one element into its allocation

# (recv_count, block) of the collective tests: a tail block that is no
# multiple of the block (pins the per-segment block grid), and whole blocks
COLL_SHAPES = [(1003, 128), (1280, 256)]


# ---- expectations ----------------------------------------------------------

def random_wires(count, block, seed):
    """Two wires as the accumulate tests build them: randn and randn * 7,
    quantized with the reference, so that block scales differ by far less
    than 2^20."""
    rng = np.random.default_rng(seed)
    return [qr.ref_wire(*qr.ref_quantize((rng.standard_normal(count) * mul).astype(F32),
                                         block))
            for mul in (1.0, 7.0)]


def exact_wire_sum(a, b, count, block, dtype):
    """Bits of dequant(a) + dequant(b) for qr.make_exact_wires wires, where
    every product and the sum are exact in float32."""
    sa, _, qa = qr.parse_wire(a, block)
    sb, _, qb = qr.parse_wire(b, block)
    s = qa.astype(F32) * sa[:, None] + qb.astype(F32) * sb[:, None]
    return qr.encode(s.reshape(-1)[:count], dtype).view(BITS[dtype])


def sum_candidates(a, b, count, block, dtype):
    """The three correct results of qa*as + qb*bs per element, as bits: both
    products rounded, or either one contracted into an fma. int8 x f32 is
    exact in float64, and with scales this close so is each sum before its
    one rounding to float32."""
    sa, _, qa = qr.parse_wire(a, block)
    sb, _, qb = qr.parse_wire(b, block)
    pa = qa.astype(F64) * sa.astype(F64)[:, None]
    pb = qb.astype(F64) * sb.astype(F64)[:, None]
    ra, rb = pa.astype(F32), pb.astype(F32)
    cands = [ra + rb, (pa + rb.astype(F64)).astype(F32), (ra.astype(F64) + pb).astype(F32)]
    return [qr.encode(c.reshape(-1)[:count], dtype).view(BITS[dtype]) for c in cands]


def matches_a_candidate(got_bits, cands):
    ok = np.zeros(got_bits.shape, dtype=bool)
    for c in cands:
        ok |= got_bits == c
    return ok


def rank_input(rank, n, dtype):
    """Rank `rank`'s send buffer: depends on the rank alone, so every rank
    can rebuild every input."""
    rng = np.random.default_rng(1000 + rank)
    return qr.encode((rng.standard_normal(n) * 3).astype(F32), dtype)


def rel_l2(got_f64, want_f64):
    return float(np.linalg.norm(got_f64 - want_f64) / max(np.linalg.norm(want_f64), 1e-30))


# ---- launcher --------------------------------------------------------------

def qrs_device(device):
    """QRS_DEVICE for run_ranks' `device`: False is the TCP transport, True
    the device transport with torch buffers, "numpy" the device transport
    with pageable numpy buffers, which the engine stages."""
    return {False: "cpu", True: "gpu", "numpy": "gpu-numpy"}[device]


def run_ranks(worker, world, device=False, timeout=120, extra_env=None, **kwargs):
    """tests.workers_quant_rs.<worker>(**kwargs) in `world` processes, on
    the TCP transport or (device=True or "numpy") all on GPU 0. Every process
    gets `timeout` seconds; the first to exceed it takes all ranks down.
    Raises on a nonzero exit; returns the stdouts."""
    port = free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ)
        env.update({"RANK": str(r), "WORLD_SIZE": str(world),
                    "MASTER_ADDR": "127.0.0.1", "MLSL_PORT": str(port),
                    "PYTHONPATH": REPO, "QRS_DEVICE": qrs_device(device)})
        if device:
            env.pop("MLSL_TRANSPORT", None)
            env["MLSL_TIMEOUT"] = "90"
        else:
            env["MLSL_TRANSPORT"] = "tcp"
        if extra_env:
            env.update(extra_env)
        procs.append(subprocess.Popen(
            [sys.executable, "-m", "tests.workers_quant_rs", worker, json.dumps(kwargs)],
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


PLUGIN = os.path.join(REPO, "build", "libquant_plugin.so")


def ensure_plugin():
    """Build the sample compression plugin once, before any rank starts."""
    if not os.path.exists(PLUGIN):
        subprocess.run(["make", "quantplugin"], cwd=REPO, check=True,
                       capture_output=True, timeout=300)


# ---- workers ---------------------------------------------------------------

class _Bufs:
    """numpy arrays on the host transport (and where QRS_DEVICE keeps them
    on the device transport), torch tensors on GPU 0 otherwise; bf16 travels
    as 16-bit integers either way."""

    def __init__(self):
        self.gpu = os.environ.get("QRS_DEVICE") == "gpu"
        if self.gpu:
            import torch
            self.torch = torch
            torch.cuda.set_device(0)

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        if not self.gpu:
            return arr.copy()
        if arr.dtype == np.uint16:
            arr = arr.view(np.int16)
        return self.torch.from_numpy(arr.copy()).cuda()

    def get(self, buf, dtype):
        if self.gpu:
            self.torch.cuda.synchronize()
            buf = buf.cpu().numpy()
        return np.ascontiguousarray(buf).view(NP_DT[dtype]).copy()


def _init():
    bufs = _Bufs()
    import mlsl_amd as mx
    mx.init()
    return mx, bufs, mx.rank(), mx.world_size()


def _reduce_scatter(mx, bufs, d, rank, size, dtype, count, inplace, starts=1):
    """`starts` runs of one persistent quantized reduce-scatter on this
    rank's input; returns the outputs and checks that an out-of-place run
    leaves the send buffer alone."""
    x = rank_input(rank, size * count, dtype)
    req = mx.PersistentRequest(d, "reduce_scatter", count, dtype=dtype, op="sum",
                               group="data", quantized=True)
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


def _configs(shapes, dtypes=("f32", "bf16"), inplace=(False, True)):
    return [(dt, c, b, ip) for dt in dtypes for c, b in shapes for ip in inplace]


def rs_check(shapes=None, dtypes=("f32", "bf16"), inplace=(False, True)):
    """World 2: every output element is one of the three candidates built
    from the reference-quantized wires of the two ranks' segments. Larger
    worlds: relative L2 error against the float64 sum below 0.05, and not
    the exact sum. World 1: dequantize(quantize(x)) bit for bit."""
    mx, bufs, rank, size = _init()
    d = mx.Distribution(size, 1)
    for dtype, count, block, inplace in _configs(shapes or COLL_SHAPES, dtypes, inplace):
        mx.set_quant_params(block)
        out = _reduce_scatter(mx, bufs, d, rank, size, dtype, count, inplace)[0]
        what = (size, dtype, count, block, "inplace" if inplace else "outofplace")
        segs = [qr.decode(rank_input(k, size * count, dtype), dtype)
                [rank * count:(rank + 1) * count] for k in range(size)]
        wires = [qr.ref_wire(*qr.ref_quantize(s, block)) for s in segs]
        if size == 1:
            want = qr.ref_dequantize(*qr.ref_quantize(segs[0], block), count, dtype)
            assert np.array_equal(out.view(BITS[dtype]), want.view(BITS[dtype])), what
        elif size == 2:
            ok = matches_a_candidate(out.view(BITS[dtype]),
                                     sum_candidates(wires[0], wires[1], count, block, dtype))
            assert ok.all(), (what, f"{(~ok).sum()} elements match no candidate")
        else:
            exact = np.sum([s.astype(F64) for s in segs], axis=0)
            rel = rel_l2(qr.decode(out, dtype).astype(F64), exact)
            print(f"rel_l2 {what}: {rel:.5f}")
            assert rel < 0.05, (what, rel)
            assert not np.array_equal(out.view(BITS[dtype]),
                                      qr.encode(exact.astype(F32), dtype).view(BITS[dtype])), \
                (what, "exact sum came back: nothing was quantized")
    d.barrier("global")
    mx.finalize()


def rs_error_feedback():
    """Eight starts of one request on the same input: the residual makes the
    mean of the outputs converge on the exact sum."""
    mx, bufs, rank, size = _init()
    d = mx.Distribution(size, 1)
    for count, block in COLL_SHAPES:
        mx.set_quant_params(block)
        outs = _reduce_scatter(mx, bufs, d, rank, size, "f32", count, False, starts=8)
        exact = np.sum([rank_input(k, size * count, "f32")[rank * count:(rank + 1) * count]
                        .astype(F64) for k in range(size)], axis=0)
        first = rel_l2(outs[0].astype(F64), exact)
        mean = rel_l2(np.mean([o.astype(F64) for o in outs], axis=0), exact)
        print(f"error feedback ({count}, {block}): first {first:.5f} mean of 8 {mean:.5f}")
        assert mean < first / 4, (count, block, first, mean)
    d.barrier("global")
    mx.finalize()


def rs_sharded_optimizer():
    """ShardedOptimizer(reduce="rs") with and without int8 compression from
    the same start: parameters stay identical across ranks, and the
    compressed step is the exact one up to the quantization error."""
    mx, bufs, rank, size = _init()
    import torch
    from mlsl_amd.parallel.zero1 import ShardedOptimizer
    dev = "cuda" if bufs.gpu else "cpu"
    d = mx.Distribution(size, 1)
    mx.set_quant_params(128)
    steps = {}
    for compression in ("none", "int8"):
        torch.manual_seed(7)
        model = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Tanh(),
                                    torch.nn.Linear(16, 4)).to(dev)   # 212 parameters
        opt = ShardedOptimizer(model.parameters(), torch.optim.SGD, d, reduce="rs",
                               compression=compression, lr=0.1)
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
    rel = rel_l2(steps["int8"], steps["none"])
    print(f"sharded optimizer step, int8 against none: rel_l2 {rel:.5f}")
    assert rel < 0.05, rel
    assert rel > 0, "int8 step equals the exact one: nothing was quantized"
    mx.set_quant_params(256)
    d.barrier("global")
    mx.finalize()


def rs_plugin():
    """Host transport with the sample compression plugin: the ABI has no
    fused hook, so the last hop is reduce_sum + dequant of the one segment;
    the residual is still per segment. Error bound as for worlds 3 and 4."""
    import ctypes
    from ctypes import byref, c_char_p, c_size_t, c_void_p
    so = PLUGIN
    assert os.path.exists(so), "build the plugin first: ensure_plugin()"
    mx, bufs, rank, size = _init()
    from mlsl_amd._lib import lib
    L = lib()

    class QP(ctypes.Structure):
        _fields_ = [("lib_path", c_char_p), ("quant", c_char_p),
                    ("dequant", c_char_p), ("reduce_sum", c_char_p),
                    ("block_size", c_size_t), ("elem_in_block", c_size_t)]

    env = c_void_p()
    assert L.mlsl_environment_get_env(byref(env)) == 0
    assert L.mlsl_environment_set_quantization_params(
        env, byref(QP(so.encode(), None, None, None, 264, 256))) == 0, \
        ctypes.string_at(L.mlsl_last_error()).decode()
    d = mx.Distribution(size, 1)
    count = 1003
    for inplace in (False, True):
        out = _reduce_scatter(mx, bufs, d, rank, size, "f32", count, inplace)[0]
        exact = np.sum([rank_input(k, size * count, "f32")[rank * count:(rank + 1) * count]
                        .astype(F64) for k in range(size)], axis=0)
        rel = rel_l2(out.astype(F64), exact)
        print(f"plugin rel_l2 world {size} inplace={inplace}: {rel:.5f}")
        assert 0 < rel < 0.05, (size, inplace, rel)
    L.mlsl_environment_set_quantization_params(
        env, byref(QP(None, None, None, None, 0, 256)))
    d.barrier("global")
    mx.finalize()


WORKERS = {
    "rs_plugin": rs_plugin,
    "rs_check": rs_check,
    "rs_error_feedback": rs_error_feedback,
    "rs_sharded_optimizer": rs_sharded_optimizer,
}


def main():
    name = sys.argv[1]
    kwargs = json.loads(sys.argv[2]) if len(sys.argv) > 2 else {}
    WORKERS[name](**kwargs)
    print(f"OK {name} rank={os.environ.get('RANK')}")


if __name__ == "__main__":
    main()
