"""The int4 accumulating all-gather: the reference, the kernel case its CPU and
GPU tests share, and the rank workers (python -m tests.workers_quant_ag4
<worker> '<json kwargs>'). Codec: tests/quant4_ref.py; buffers and transport:
tests/workers_quant_rs.py. Every rank checks against the same numpy reference,
bit for bit, so the ranks agree among themselves."""
import functools
import json
import os
import subprocess
import sys

import numpy as np

from tests import quant4_ref as q4
from tests import workers_quant4 as w4
from tests import workers_quant_rs as w
from tests.mp import REPO, free_port

qr, F32 = q4.qr, np.float32
ITEM, NP_DT, BITS = w.ITEM, w.NP_DT, w.BITS

# (nseg, count, block, elements `out` is offset by, bytes the wire is offset by)
CASES = [(1, 256, 256, 0, 0),    # one whole block
         (3, 301, 256, 0, 0),    # segments 1, 2 misaligned; 45 = 5 words + 5 elements
         (8, 8, 8, 0, 0),        # one word per block, 12-byte wire blocks
         (9, 520, 256, 0, 0),    # nine segments; a partial block of whole words
         (2, 1100, 1024, 0, 0),  # 128 words per block: two words per lane
         (3, 512, 256, 1, 0),    # `out` misaligned: generic only, "fast" raises
         (3, 512, 256, 0, 8)]    # fast path, the wire 8-byte aligned only


def trip_case(fast):
    # three segments of a third of one launch's grid plus two blocks: the second
    # trip starts inside segment 2, its waves' first blocks lie in segment 0
    from mlsl_amd import ops
    nb = ops.quant4_blocks_per_trip(fast) // 3 + 2
    return (3, nb * 256, 256, 0, 0) if fast else (3, nb * 64 - 5, 64, 0, 0)


def ref_segments(wire, nseg, count, block, dtype, base=None):
    """Bits of out[j * count + i] = encode(q * scale), or with `base` (what
    `out` held) encode(fma(q, scale, decode(base))), over nseg segment wires."""
    s, _, q = q4.unpack(wire, block)
    q = q.reshape(nseg, -1)[:, :count]
    s = np.repeat(s.reshape(nseg, -1), block, axis=1)[:, :count]
    v = (q.astype(F32) * s if base is None
         else q4.fma(q, s, qr.decode(base, dtype).reshape(nseg, count)))
    return qr.encode(v.reshape(-1), dtype).view(BITS[dtype])


def base_values(n, dtype, seed):
    rng = np.random.default_rng(seed)   # non-zero: what an accumulate adds to
    return qr.encode((rng.uniform(0.25, 4.0, n) * rng.choice([-1.0, 1.0], n)).astype(F32), dtype)


@functools.lru_cache(maxsize=None)
def expectation(nseg, count, block, dtype, acc):
    wire = np.concatenate(q4.make_wires(nseg, count, block, seed=count + nseg))
    base = base_values(nseg * count, dtype, count)
    return wire, base, ref_segments(wire, nseg, count, block, dtype, base if acc else None)


def run_case(gpu, case, dtype, acc, path=None):
    """ops.dequantize_segments4 (gpu) or its host twin, `out` and the wire
    between sentinels; returns out's bits, checked against the reference."""
    from mlsl_amd import ops
    nseg, count, block, off, wfront = case
    wire, base, want = expectation(nseg, count, block, dtype, acc)
    lo, n = qr.GUARD + off * ITEM[dtype], nseg * count * ITEM[dtype]
    out = np.full(lo + n + qr.GUARD, 0xCD, dtype=np.uint8)
    out[lo:lo + n] = base.view(np.uint8) if acc else 0xAB
    wimg = np.full(wfront + wire.size + qr.GUARD, 0xCD, dtype=np.uint8)
    wimg[wfront:wfront + wire.size] = wire
    kw = dict(block=block, dtype=dtype, accumulate=acc)
    if gpu:
        import torch
        d_out, d_wire = torch.from_numpy(out).cuda(), torch.from_numpy(wimg).cuda()
        assert d_out.data_ptr() % 16 == 0 and d_wire.data_ptr() % 16 == 0
        ops.dequantize_segments4(d_wire[wfront:wfront + wire.size], d_out[lo:lo + n], count,
                                 nseg, path=path, **kw)
        torch.cuda.synchronize()
        got, got_wire = d_out.cpu().numpy(), d_wire.cpu().numpy()
    else:
        got, got_wire = out.copy(), wimg.copy()
        ops.host_dequantize_segments4(got_wire[wfront:wfront + wire.size],
                                      got[lo:lo + n].view(NP_DT[dtype]), count, nseg, **kw)
    assert np.array_equal(got_wire, wimg), "wire modified, or a write around it"
    assert (np.delete(got, np.s_[lo:lo + n]) == 0xCD).all(), "write outside out"
    bits = got[lo:lo + n].view(BITS[dtype]).copy()
    assert np.array_equal(bits, want), (case, dtype, acc, path, int((bits != want).sum()))
    return bits


def run_ranks(worker, world, device=False, extra_env=None, **kwargs):
    env = dict(os.environ, WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
               MLSL_PORT=str(free_port()), PYTHONPATH=REPO, QRS_DEVICE=w.qrs_device(device),
               **(extra_env or {}))
    env.pop("MLSL_TRANSPORT", None)
    env.update({"MLSL_TIMEOUT": "90"} if device else {"MLSL_TRANSPORT": "tcp"})
    procs = [subprocess.Popen(
        [sys.executable, "-m", "tests.workers_quant_ag4", worker, json.dumps(kwargs)],
        env=dict(env, RANK=str(r)), cwd=REPO, stdout=subprocess.PIPE,
        stderr=subprocess.STDOUT, text=True) for r in range(world)]
    try:
        outs = [p.communicate(timeout=120)[0] for p in procs]
    finally:
        for p in procs:
            p.kill()    # a rank that timed out takes the others down
    failed = [f"--- rank {r} rc={p.returncode} ---\n{o[-3000:]}"
              for r, (p, o) in enumerate(zip(procs, outs)) if p.returncode != 0]
    assert not failed, f"{worker} world={world} failed:\n" + "\n".join(failed)


def ag4_check():
    """Two starts of one accumulating bits=4 all_gather: after each, recv is
    the reference fma of every rank's quant4_ref wire onto the old recv."""
    mx, bufs, rank, size = w._init()
    d = mx.Distribution(size, 1)
    for dtype in ("f32", "bf16"):
        for count, block in ((1300, 256), (64, 8)):
            mx.set_quant_params(block)
            wire = np.concatenate([q4.codec(w.rank_input(r, count, dtype), None, count, block,
                                            dtype)["wire"] for r in range(size)])
            req = mx.PersistentRequest(d, "all_gather", count, dtype=dtype, group="data",
                                       quantized=True, accumulate=True, bits=4)
            want = base_values(size * count, dtype, 77)
            recv, x = bufs.put(want), w.rank_input(rank, count, dtype)
            for start in range(2):
                send = bufs.put(x)
                req.start(send, recv)
                req.wait()
                got = bufs.get(recv, dtype).view(BITS[dtype])
                want = ref_segments(wire, size, count, block, dtype, want.view(NP_DT[dtype]))
                assert np.array_equal(got, want), (size, dtype, count, start,
                                                   int((got != want).sum()))
            req.destroy()
    mx.set_quant_params(256)
    d.barrier("global")
    mx.finalize()


def refusals():
    """What the 4-bit all_gather refuses at creation, by message."""
    import ctypes
    mx, bufs, rank, size = w._init()
    import torch
    from mlsl_amd._lib import lib
    from mlsl_amd.parallel.zero1 import ShardedOptimizer
    d = mx.Distribution(size, 1)

    def mk(dtype="f32", accumulate=True):
        return lambda: mx.PersistentRequest(d, "all_gather", 64, dtype=dtype, group="data",
                                            quantized=True, bits=4, accumulate=accumulate)
    w4._raises(ValueError, 'bits=4 is not wired to kind="all_gather"', mk(accumulate=False))
    w4._raises(ValueError, "accumulate=True only", mk(accumulate=False))
    w4._raises(RuntimeError, "f32/bf16 only", mk("f64"))
    mx.set_quant_params(12)
    w4._raises(RuntimeError, "multiple of 8 at 4 bits", mk())
    mx.set_quant_params(256)
    QP = type("QP", (ctypes.Structure,), {"_fields_": [
        (f, ctypes.c_char_p) for f in ("lib_path", "quant", "dequant", "reduce_sum")] + [
        ("block_size", ctypes.c_size_t), ("elem_in_block", ctypes.c_size_t)]})
    env = ctypes.c_void_p()
    assert lib().mlsl_environment_get_env(ctypes.byref(env)) == 0
    assert lib().mlsl_environment_set_quantization_params(
        env, ctypes.byref(QP(w.PLUGIN.encode(), None, None, None, 264, 256))) == 0
    w4._raises(RuntimeError, "4-bit wire codec cannot run with a compression plugin", mk())
    lib().mlsl_environment_set_quantization_params(
        env, ctypes.byref(QP(None, None, None, None, 0, 256)))
    for text in ("'none'", "'int8'", "'int4'"):
        w4._raises(ValueError, text, lambda: ShardedOptimizer(
            [torch.nn.Parameter(torch.zeros(8))], torch.optim.SGD, d, ag_compression="fp8"))
    d.barrier("global")
    mx.finalize()


def zero1_check(compression="none", zero_steps=0):
    """ShardedOptimizer(ag_compression="int4"), SGD on 1003 f32 parameters
    (padded to the shards), blocks of 128: three steps against a numpy
    emulation, bit for bit: delta = master - replica, quant4_ref's codec
    without a residual, fma onto the replica; master is the exact shard step
    (lr and 1 / world are powers of two, the gradients multiples of 1/8: sums
    and products are exact). Then `zero_steps` steps with zero gradients: per
    wire block max|master - replica| is at most the one before the step / 14
    (scale = max / 7, round to nearest) plus half an ulp of the replica's
    largest magnitude there (the fma's rounding). The numpy emulation alone
    stays within that bound for these inputs."""
    mx, bufs, rank, size = w._init()
    import torch
    from mlsl_amd.parallel.zero1 import ShardedOptimizer
    d = mx.Distribution(size, 1)
    n, block, lr, dev = 1003, 128, 0.5, "cuda" if bufs.gpu else "cpu"
    mx.set_quant_params(block)
    p0 = w.rank_input(99, n, "f32")
    param = torch.nn.Parameter(torch.from_numpy(p0.copy()).to(dev))
    opt = ShardedOptimizer([param], torch.optim.SGD, d, reduce="rs", compression=compression,
                           ag_compression="int4", lr=lr)
    shard = opt.shard
    assert shard * size > n and opt.master is not None
    replica = np.zeros(shard * size, dtype=F32)
    replica[:n] = p0
    master = replica.copy()
    errs = [np.zeros(shard * size, dtype=F32) for _ in range(size)]
    for step in range(3 + zero_steps):
        grads = [np.zeros(shard * size, dtype=F32) for _ in range(size)]
        for k in range(size if step < 3 else 0):
            rng = np.random.default_rng(10 * step + k)
            grads[k][:n] = np.rint(np.clip(rng.standard_normal(n) * 8, -24, 24)) / 8
        param.grad = torch.from_numpy(grads[rank][:n].copy()).to(dev)
        opt.step()
        if compression == "int4":
            wires = w4.quantize_all("reduce_scatter", grads, errs, shard, block, "f32")
            g = np.concatenate([w4.finish("reduce_scatter", wires, r, shard, block, "f32")
                                for r in range(size)])
        else:
            g = sum(grads)
        master = master + F32(-lr) * (g / F32(size))
        wire = np.concatenate([q4.codec((master - replica)[r * shard:(r + 1) * shard], None,
                                        shard, block, "f32")["wire"] for r in range(size)])
        new = ref_segments(wire, size, shard, block, "f32", replica).view(F32)
        got = opt.flat.detach().cpu().numpy()
        assert np.array_equal(got.view(np.uint32), new.view(np.uint32)), (size, step)
        own = slice(rank * shard, (rank + 1) * shard)
        assert np.array_equal(opt.master.cpu().numpy().view(np.uint32),
                              master[own].view(np.uint32)), (size, step)
        if step >= 3:
            before = np.abs(master.astype(np.float64) - replica)
            after = np.abs(master.astype(np.float64) - got)
            for lo in [s + b for s in range(0, shard * size, shard)
                       for b in range(0, shard, block)]:
                blk = slice(lo, min(lo + block, (lo // shard + 1) * shard))
                bound = before[blk].max() / 14 + np.spacing(np.abs(got[blk]).max()) / 2
                assert after[blk].max() <= bound, (step, lo, after[blk].max(), bound)
        replica = new
    mx.set_quant_params(256)
    d.barrier("global")
    mx.finalize()


if __name__ == "__main__":
    {f.__name__: f for f in (ag4_check, refusals, zero1_check)}[sys.argv[1]](
        **(json.loads(sys.argv[2]) if len(sys.argv) > 2 else {}))
    print(f"OK {sys.argv[1]} rank={os.environ.get('RANK')}")
