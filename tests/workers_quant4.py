"""Rank workers of the int4 collectives' tests (python -m tests.workers_quant4
<worker> '<json kwargs>'). Inputs are a function of the rank, so every rank
computes the bytes it expects from the host twins. Buffers and transport as in
tests/workers_quant_rs.py, whose launcher is tied to its own module."""
import json
import os
import subprocess
import sys

import numpy as np

from tests import workers_quant_rs as w
from tests.mp import REPO, free_port

NP_DT, BITS = w.NP_DT, w.BITS
# 1003 at block 128: 8 units, the last partial; owner ranges 2, 3, 3 on 3 ranks
SHAPES = [(1003, 128), (1280, 256)]
# the variables choose between int8 algorithms: a 4-bit request ignores them
ENV = {"MLSL_QUANT_AR_ALGO": "ring", "MLSL_QUANT_RS_ALGO": "ring"}


def run_ranks(worker, world, device=False, timeout=120, **kwargs):
    port, procs = free_port(), []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MLSL_PORT=str(port), PYTHONPATH=REPO, QRS_DEVICE=w.qrs_device(device), **ENV)
        env.pop("MLSL_TRANSPORT", None)
        env.update({"MLSL_TIMEOUT": "90"} if device else {"MLSL_TRANSPORT": "tcp"})
        procs.append(subprocess.Popen(
            [sys.executable, "-m", "tests.workers_quant4", worker, json.dumps(kwargs)],
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


def quantize_all(kind, xs, errs, count, block, dtype):
    """One start's wires of the inputs `xs`, one per rank; `errs` advance."""
    from mlsl_amd import ops
    nseg, wb = len(xs) if kind == "reduce_scatter" else 1, ops.wire_bytes(count, block, 4)
    wires = [np.zeros(nseg * wb, dtype=np.uint8) for _ in xs]
    for x, e, wire in zip(xs, errs, wires):
        for j in range(nseg):
            seg = slice(j * count, (j + 1) * count)
            ops.host_quantize4(x[seg], wire[j * wb:(j + 1) * wb], count, err=e[seg],
                               block=block, dtype=dtype)
    return wires


def finish(kind, wires, rank, count, block, dtype):
    """Rank `rank`'s output: the wires summed in rank order, requantized once
    for the all_reduce (into wires[0]), dequantized."""
    from mlsl_amd import ops
    size, wb = len(wires), ops.wire_bytes(count, block, 4)
    out = np.zeros(count, dtype=NP_DT[dtype])
    if kind == "reduce_scatter" and size > 1:
        ops.host_quant_sum_dequant_n4([x[rank * wb:(rank + 1) * wb] for x in wires], out,
                                      count, block=block, dtype=dtype)
        return out
    if size > 1:
        ops.host_quant_sum_requant_n4(wires, wires[0], wb // (block // 2 + 8), block=block)
    ops.host_dequantize4(wires[0], out, count, block=block, dtype=dtype)
    return out


def coll_check(kind):
    """Two starts of a bits=4 request naming no algorithm; residual carried."""
    mx, bufs, rank, size = w._init()
    d = mx.Distribution(size, 1)
    for dtype in ("f32", "bf16"):
        for count, block in SHAPES:
            mx.set_quant_params(block)
            n_in = count * (size if kind == "reduce_scatter" else 1)
            xs = [w.rank_input(k, n_in, dtype) for k in range(size)]
            errs = [np.zeros(n_in, dtype=NP_DT[dtype]) for _ in range(size)]
            req = mx.PersistentRequest(d, kind, count, dtype=dtype, op="sum", group="data",
                                       quantized=True, bits=4)
            for start in range(2):
                send, recv = bufs.put(xs[rank]), bufs.put(np.zeros(count, dtype=NP_DT[dtype]))
                req.start(send, recv)
                req.wait()
                want = finish(kind, quantize_all(kind, xs, errs, count, block, dtype), rank,
                              count, block, dtype)
                bad = int((bufs.get(recv, dtype).view(BITS[dtype]) != want.view(BITS[dtype])).sum())
                assert bad == 0, (kind, size, dtype, count, block, start, f"{bad} differ")
            req.destroy()
    mx.set_quant_params(256)
    d.barrier("global")
    mx.finalize()


def _raises(exc, text, f):
    try:
        f()
    except exc as e:
        assert text in str(e), (text, str(e))
    else:
        raise AssertionError(f"no {exc.__name__} with {text!r}")


def refusals(plugin=False):
    """What bits=4 refuses at creation, by message."""
    mx, bufs, rank, size = w._init()
    import torch
    from mlsl_amd.parallel.zero1 import ShardedOptimizer
    d = mx.Distribution(size, 1)

    def mk(kind="all_reduce", bits=4, **kw):
        return lambda: mx.PersistentRequest(d, kind, 64, dtype="f32", op="sum", group="data",
                                            quantized=True, bits=bits, **kw)
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
        _raises(RuntimeError, "plugin", mk())
        lib().mlsl_environment_set_quantization_params(
            env, ctypes.byref(QP(None, None, None, None, 0, 256)))
    if size > 8:
        _raises(RuntimeError, "at most 8 ranks per group (its requantize takes 8 wires); use "
                "bits=8", mk())
        _raises(RuntimeError, "at most 8 ranks per group (its fan-in takes 8 wires); use "
                "bits=8", mk("reduce_scatter"))
    _raises(RuntimeError, "does not run the ring", mk(ar_algo="ring"))
    _raises(RuntimeError, "does not run the ring", mk("reduce_scatter", algo="ring"))
    _raises(ValueError, 'bits=4 is not wired to kind="all_gather"', mk("all_gather"))
    _raises(ValueError, "4 or 8 payload bits", mk(bits=5))
    _raises(TypeError, "bits", lambda: mx.SegmentedAllReduce(d, [8], bits=4))
    _raises(TypeError, "bits", lambda: mx.SegmentedReduceScatter(d, [8], bits=4))
    mx.set_quant_params(12)
    _raises(RuntimeError, "multiple of 8 at 4 bits", mk())
    mx.set_quant_params(256)
    so = lambda **kw: lambda: ShardedOptimizer(  # noqa: E731
        [torch.nn.Parameter(torch.zeros(8))], torch.optim.SGD, d, reduce="rs",
        compression="int4", lr=0.5, **kw)
    _raises(ValueError, 'does not run rs_algo="ring"', so(rs_algo="ring"))
    _raises(ValueError, 'not wired to grads="in_place"', so(grads="in_place"))
    d.barrier("global")
    mx.finalize()


def sharded_optimizer(n=1003, block=128, lr=0.5, steps=3):
    """Three SGD steps against a replay from the host twins. lr and 1/world are
    powers of two: the update's products are exact, fused or not."""
    mx, bufs, rank, size = w._init()
    import torch
    from mlsl_amd.parallel.zero1 import ShardedOptimizer
    d = mx.Distribution(size, 1)
    mx.set_quant_params(block)
    p0 = w.rank_input(99, n, "f32")
    param = torch.nn.Parameter(torch.from_numpy(p0.copy()).to("cuda" if bufs.gpu else "cpu"))
    opt = ShardedOptimizer([param], torch.optim.SGD, d, reduce="rs", compression="int4",
                           lr=lr)
    shard = opt.shard
    flat = np.zeros(shard * size, dtype=np.float32)
    flat[:n] = p0
    errs = [np.zeros(shard * size, dtype=np.float32) for _ in range(size)]
    for step in range(steps):
        grads = [np.zeros(shard * size, dtype=np.float32) for _ in range(size)]
        for k in range(size):
            grads[k][:n] = w.rank_input(10 * step + k, n, "f32")
        param.grad = torch.from_numpy(grads[rank][:n].copy()).to(param.device)
        opt.step()
        wires = quantize_all("reduce_scatter", grads, errs, shard, block, "f32")
        for r in range(size):
            g = finish("reduce_scatter", wires, r, shard, block, "f32")
            own = slice(r * shard, (r + 1) * shard)
            flat[own] = flat[own] + np.float32(-lr) * (g / np.float32(size))
        got = opt.flat.detach().cpu().numpy()
        assert np.array_equal(got.view(np.uint32), flat.view(np.uint32)), (size, step)
    mx.set_quant_params(256)
    d.barrier("global")
    mx.finalize()


if __name__ == "__main__":
    {f.__name__: f for f in (coll_check, refusals, sharded_optimizer)}[sys.argv[1]](
        **(json.loads(sys.argv[2]) if len(sys.argv) > 2 else {}))
    print(f"OK {sys.argv[1]} rank={os.environ.get('RANK')}")
