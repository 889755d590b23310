"""Two-shot quantized allreduce: what its tests share, and their rank workers.

The two-shot algorithm quantizes every contribution once, sends each range of
wire units to its owner, sums the N wires of a range in rank order with one
fma per wire, requantizes the sum once, gathers the ranges and dequantizes
the whole wire on every rank. Its result is therefore a fixed function of the
inputs at any world size, the same on all ranks: `expected_allreduce`.
Helpers, shapes and inputs come from tests/workers_quant_rs.py,
tests/workers_quant_rs_direct.py and tests/quant_ref.py; this module adds the
N-way sum-requantize reference, the kernel cases, a launcher for its own
workers, and the workers (TCP host transport with numpy buffers, or every
rank on GPU 0 with torch buffers; QRS_DEVICE picks).

Run as: python -m tests.workers_quant_ar <worker> '<json kwargs>'
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
from tests import workers_quant_rs_direct as wd
from tests.mp import REPO, free_port

F32, F64 = np.float32, np.float64
ITEM, NP_DT, BITS = w.ITEM, w.NP_DT, w.BITS
SENTINEL = 0xCD
# wires sit 8 but not 16 bytes into their (16-byte aligned) allocations, as
# TMP slots do, which start at multiples of 264 bytes
WIRE_FRONT = 8


# ---- expectations ----------------------------------------------------------

def ref_sum_requant_n(wires, nunits, block):
    """Wire bytes of the N-way sum-requantize over `nunits` whole units: the
    float32 sums of `ref_sum_dequant_n` (which asserts that the scale ratios
    stay below 2^16, where it is exact), requantized by the pinned codec."""
    acc = wd.ref_sum_dequant_n(wires, nunits * block, block, "f32").view(F32)
    return qr.ref_wire(*qr.ref_quantize(acc, block))


def seg_offset(units, parts, i):
    return i * units // parts


def seg_count(units, parts, i):
    return (i + 1) * units // parts - i * units // parts


def expected_allreduce(size, count, block, dtype):
    """Bits of every rank's output of a two-shot allreduce's first start (zero
    residual) on w.rank_input: every input quantized whole, the unit range of
    each owner summed over the ranks in ascending order and requantized once,
    the ranges concatenated and dequantized."""
    ins = [qr.decode(w.rank_input(k, count, dtype), dtype) for k in range(size)]
    wires = [qr.ref_wire(*qr.ref_quantize(x, block)) for x in ins]
    if size == 1:
        s, _, q = qr.parse_wire(wires[0], block)
        return qr.ref_dequantize(s, q, count, dtype).view(BITS[dtype])
    units, unit = qr.nblocks(count, block), block + qr.HDR
    parts = []
    for owner in range(size):
        lo, n = seg_offset(units, size, owner), seg_count(units, size, owner)
        if n:
            parts.append(ref_sum_requant_n([x[lo * unit:(lo + n) * unit] for x in wires],
                                           n, block))
    s, _, q = qr.parse_wire(np.concatenate(parts), block)
    return qr.ref_dequantize(s, q, count, dtype).view(BITS[dtype])


def exact_allreduce(size, count, dtype):
    return np.sum([qr.decode(w.rank_input(k, count, dtype), dtype).astype(F64)
                   for k in range(size)], axis=0)


# ---- kernel cases ----------------------------------------------------------

KERNEL_NWIRES = [1, 2, 3, 8]
# (units, block): generic scalar-free path at a small and a mid block, two
# vector passes per block at 512, the fast path with an even count and with
# the last pair's second half idle
SMALL_CASES = [(3, 8), (8, 128), (10, 512), (4, 256), (5, 256)]
# a second trip round the grid-stride loop: the fast path covers 16384 units
# per pass, the generic path 8192
MULTIPASS_CASES = [(16387, 256), (8195, 128)]
MULTIPASS_NWIRES = 3
KERNEL_PARAMS = ([(u, b, n) for u, b in SMALL_CASES for n in KERNEL_NWIRES] +
                 [(u, b, MULTIPASS_NWIRES) for u, b in MULTIPASS_CASES])
# (units, block, nwires, k): the destination is wire k
ALIAS_PARAMS = [(u, b, n, k) for u, b in SMALL_CASES for n in KERNEL_NWIRES
                for k in sorted({0, n - 1})]


def kernel_wires(nwires, units, block):
    """wd.kernel_wires over whole units: scales spread over [1, 7]. Cached
    there: treat as read-only."""
    return wd.kernel_wires(nwires, units * block, block)


@functools.lru_cache(maxsize=None)
def kernel_expectation(nwires, units, block):
    want = ref_sum_requant_n(kernel_wires(nwires, units, block), units, block)
    want.setflags(write=False)
    return want


TIE_UNIT, ZERO_UNIT = 0, 1


@functools.lru_cache(maxsize=None)
def constructed_wires(block):
    """Two wires of three units. Unit 0 is a tie block: wire a has scale 2^-3,
    q[0] = 127 and |q| <= 126 elsewhere; wire b has scale 2^-4, q[0] = 0 and
    q = +-1 elsewhere. Every sum is (k +- 0.5) * 2^-3 under a block maximum of
    127 * 2^-3, so the new scale is 2^-3 and every element but the first is a
    rounding tie. Unit 1 is zero in both wires. Unit 2 is random."""
    rng = np.random.default_rng(block)
    a, b = (np.array(x) for x in wd.kernel_wires(2, 3 * block, block))
    sa, _, qa = (np.array(x) for x in qr.parse_wire(a, block))
    sb, _, qb = (np.array(x) for x in qr.parse_wire(b, block))
    sa[TIE_UNIT], sb[TIE_UNIT] = 2.0 ** -3, 2.0 ** -4
    qa[TIE_UNIT] = rng.integers(-126, 127, block)
    qa[TIE_UNIT, 0] = 127
    qb[TIE_UNIT] = np.where(rng.integers(0, 2, block) == 0, -1, 1)
    qb[TIE_UNIT, 0] = 0
    qa[ZERO_UNIT], qb[ZERO_UNIT] = 0, 0
    out = (qr.ref_wire(sa, qa), qr.ref_wire(sb, qb))
    for x in out:
        x.setflags(write=False)
    return out


def check_constructed(got, block):
    """What the constructed units must requantize to, spelled out."""
    a, b = constructed_wires(block)
    _, _, qa = qr.parse_wire(a, block)
    _, _, qb = qr.parse_wire(b, block)
    s, w1, q = qr.parse_wire(got, block)
    assert s[TIE_UNIT] == F32(2.0 ** -3) and s[ZERO_UNIT] == F32(1.0), s[:2]
    assert (w1 == 0).all() and not np.signbit(w1).any(), "header word 1"
    assert (q[ZERO_UNIT] == 0).all()
    # (k +- 0.5) rounds to the even neighbour
    ties = qa[TIE_UNIT].astype(F64) + qb[TIE_UNIT].astype(F64) / 2
    assert (np.abs(ties[1:] - np.floor(ties[1:])) == 0.5).all()
    assert np.array_equal(q[TIE_UNIT], np.rint(ties).astype(np.int8))
    assert np.array_equal(got, ref_sum_requant_n([a, b], 3, block))


def order_case(run):
    """Three wires big, tiny, tiny and tiny, tiny, big through
    run(wires, nunits, block). In float32, 1 + 2^-24 + 2^-24 is 1 when the
    small terms come last, one at a time, and 1 + 2^-23 when they come first
    (the scales are 2^24 apart, so ref_sum_dequant_n does not apply and the
    sums are written out here); each result must be the pinned codec's wire
    of its sum. Returns the two results, which differ."""
    block = 8
    big = qr.ref_wire(np.array([1.0], F32), np.full((1, block), 1, np.int8))
    tiny = qr.ref_wire(np.array([2.0 ** -24], F32), np.full((1, block), 1, np.int8))
    got = []
    for order, total in (([big, tiny, tiny], F32(1.0)),
                         ([tiny, tiny, big], F32(1.0) + F32(2.0 ** -23))):
        got.append(run(order, 1, block))
        want = qr.ref_wire(*qr.ref_quantize(np.full(block, total, dtype=F32), block))
        assert np.array_equal(got[-1], want), order
    return got


def _guarded_wire(x):
    """`x` WIRE_FRONT bytes into a sentinel-filled allocation with GUARD
    sentinel bytes behind it."""
    g = np.full(WIRE_FRONT + x.size + qr.GUARD, SENTINEL, dtype=np.uint8)
    g[WIRE_FRONT:WIRE_FRONT + x.size] = x
    return g


def check_guarded(g, x, what):
    """Sentinels around a guarded wire intact and, with `x`, content equal."""
    n = g.size - WIRE_FRONT - qr.GUARD
    assert (g[:WIRE_FRONT] == SENTINEL).all() and (g[WIRE_FRONT + n:] == SENTINEL).all(), \
        f"write around {what}"
    if x is not None:
        assert np.array_equal(g[WIRE_FRONT:WIRE_FRONT + n], x), f"{what} modified"


def run_sum_requant_n(launch, to_dev, to_host, wires, nunits, block, alias=None):
    """launch(wire_views, dst_view, nunits, block) on guarded buffers made by
    to_dev from numpy and read back by to_host. `alias` = k makes wire k the
    destination. Checks the sentinels and that no input but the destination
    changed; returns the destination's bytes."""
    n = nunits * (block + qr.HDR)
    bufs = [to_dev(_guarded_wire(x)) for x in wires]
    views = [b[WIRE_FRONT:WIRE_FRONT + n] for b in bufs]
    if alias is None:
        dst_buf = to_dev(_guarded_wire(np.full(n, 0xAB, dtype=np.uint8)))
        dst = dst_buf[WIRE_FRONT:WIRE_FRONT + n]
    else:
        dst_buf, dst = bufs[alias], views[alias]
    launch(views, dst, nunits, block)
    for k, (b, x) in enumerate(zip(bufs, wires)):
        check_guarded(to_host(b), None if k == alias else x, f"wire {k}")
    out = to_host(dst_buf)
    check_guarded(out, None, "dst")
    return out[WIRE_FRONT:WIRE_FRONT + n].copy()


def host_sum_requant_n(wires, nunits, block, alias=None):
    from mlsl_amd import ops
    return run_sum_requant_n(
        lambda ws, d, u, b: ops.host_quant_sum_requant_n(ws, d, u, block=b),
        lambda a: a, lambda a: a, wires, nunits, block, alias)


# ---- launcher --------------------------------------------------------------

def run_ranks(worker, world, device=False, timeout=120, extra_env=None, **kwargs):
    """tests.workers_quant_ar.<worker>(**kwargs) in `world` processes, on the
    TCP transport or (device=True or "numpy") all on GPU 0. Every process gets
    `timeout` seconds; the first to exceed it takes all ranks down. Raises on
    a nonzero exit; returns the stdouts."""
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
            [sys.executable, "-m", "tests.workers_quant_ar", worker, json.dumps(kwargs)],
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


digests = wd.digests


def assert_ranks_agree(outs, world, configs):
    """Every rank printed `configs` digests and they are the same on all."""
    found = digests(outs)
    assert sorted(found) == list(range(world)), sorted(found)
    assert all(len(v) == configs for v in found.values()), found
    assert all(v == found[0] for v in found.values()), "outputs differ across ranks"
    return found


# ---- workers ---------------------------------------------------------------

def _all_reduce(mx, bufs, d, rank, size, dtype, count, inplace, ar_algo, starts=1):
    """`starts` runs of one persistent quantized allreduce with `ar_algo` on
    this rank's input; returns the outputs and checks that an out-of-place
    run leaves the send buffer alone."""
    x = w.rank_input(rank, count, dtype)
    req = mx.PersistentRequest(d, "all_reduce", count, dtype=dtype, op="sum",
                               group="data", quantized=True, ar_algo=ar_algo)
    outs = []
    for _ in range(starts):
        send = bufs.put(x)
        recv = send if inplace else bufs.put(np.zeros(count, dtype=NP_DT[dtype]))
        req.start(send, recv)
        req.wait()
        outs.append(bufs.get(recv, dtype))
        if not inplace:
            assert np.array_equal(bufs.get(send, dtype), x), "send buffer modified"
    req.destroy()
    return outs


def twoshot_check(shapes=None, dtypes=("f32", "bf16"), ar_algo="two_shot",
                  compare_ring=True, inplace=(False, True)):
    """The first start of a two-shot request equals `expected_allreduce` bit
    for bit on every rank (world 1: dequantize(quantize(x))); a digest of each
    output is printed so that the launcher can compare ranks. From world 3 up
    the ring, on the same inputs, is further from the float64 sum: it
    requantizes every segment N-1 times. `ar_algo=None` relies on
    MLSL_QUANT_AR_ALGO=two_shot in the environment."""
    mx, bufs, rank, size = w._init()
    d = mx.Distribution(size, 1)
    for dtype, count, block, inplace in w._configs([tuple(s) for s in shapes or w.COLL_SHAPES],
                                                   dtypes, inplace):
        mx.set_quant_params(block)
        out = _all_reduce(mx, bufs, d, rank, size, dtype, count, inplace, ar_algo)[0]
        what = (size, dtype, count, block, "inplace" if inplace else "outofplace")
        want = expected_allreduce(size, count, block, dtype)
        bad = int((out.view(BITS[dtype]) != want).sum())
        assert bad == 0, (what, f"{bad} of {count} elements differ from the reference")
        print(f"DIGEST {rank} {hashlib.sha256(out.tobytes()).hexdigest()}")
        if size >= 3 and compare_ring:
            ring = _all_reduce(mx, bufs, d, rank, size, dtype, count, inplace, "ring")[0]
            exact = exact_allreduce(size, count, dtype)
            e_two = w.rel_l2(qr.decode(out, dtype).astype(F64), exact)
            e_ring = w.rel_l2(qr.decode(ring, dtype).astype(F64), exact)
            print(f"rel_l2 {what}: two_shot {e_two:.5f} ring {e_ring:.5f} "
                  f"ratio {e_ring / e_two:.3f}")
            assert e_two < e_ring, (what, e_two, e_ring)
    mx.set_quant_params(256)
    d.barrier("global")
    mx.finalize()


def twoshot_error_feedback():
    """Eight starts of one two-shot request on the same input: the residual
    carries the first quantization's error (not the requantization's), and
    the mean of the outputs is closer to the exact sum than the first by a
    factor of at least 1.5."""
    mx, bufs, rank, size = w._init()
    d = mx.Distribution(size, 1)
    for count, block in w.COLL_SHAPES:
        mx.set_quant_params(block)
        outs = _all_reduce(mx, bufs, d, rank, size, "f32", count, False, "two_shot",
                           starts=8)
        exact = exact_allreduce(size, count, "f32")
        first = w.rel_l2(outs[0].astype(F64), exact)
        mean = w.rel_l2(np.mean([o.astype(F64) for o in outs], axis=0), exact)
        print(f"error feedback ({count}, {block}): first {first:.5f} mean of 8 {mean:.5f} "
              f"factor {first / mean:.3f}")
        assert mean * 1.5 <= first, (count, block, first, mean)
    mx.set_quant_params(256)
    d.barrier("global")
    mx.finalize()


def digest_outputs(ar_algo=None):
    """Print a digest of every configuration's first-start output, for tests
    that compare two launches (with and without MLSL_QUANT_AR_ALGO)."""
    mx, bufs, rank, size = w._init()
    d = mx.Distribution(size, 1)
    for dtype, count, block, inplace in w._configs(w.COLL_SHAPES):
        mx.set_quant_params(block)
        out = _all_reduce(mx, bufs, d, rank, size, dtype, count, inplace, ar_algo)[0]
        print(f"DIGEST {rank} {hashlib.sha256(out.tobytes()).hexdigest()}")
    mx.set_quant_params(256)
    d.barrier("global")
    mx.finalize()


def twoshot_too_large(env_choice=False):
    """More than 8 ranks: the request fails at creation, names the limit and
    the ring, and the variable when the choice came from it; the ring still
    builds."""
    mx, bufs, rank, size = w._init()
    assert size > 8
    d = mx.Distribution(size, 1)
    try:
        mx.PersistentRequest(d, "all_reduce", 256, dtype="f32", op="sum", group="data",
                             quantized=True, ar_algo=None if env_choice else "two_shot")
    except RuntimeError as e:
        assert "at most 8 ranks" in str(e) and "use the ring" in str(e), str(e)
        assert ("MLSL_QUANT_AR_ALGO" in str(e)) == env_choice, str(e)
    else:
        raise AssertionError("two-shot request on 9 ranks was created")
    mx.PersistentRequest(d, "all_reduce", 256, dtype="f32", op="sum", group="data",
                         quantized=True, ar_algo="ring").destroy()
    d.barrier("global")
    mx.finalize()


def twoshot_plugin():
    """With a compression plugin the two-shot request fails at creation: the
    plugin ABI has no N-way sum. The ring still builds."""
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
        mx.PersistentRequest(d, "all_reduce", 1003, dtype="f32", op="sum", group="data",
                             quantized=True, ar_algo="two_shot")
    except RuntimeError as e:
        assert "plugin" in str(e) and "use the ring" in str(e), str(e)
    else:
        raise AssertionError("two-shot request with a compression plugin was created")
    mx.PersistentRequest(d, "all_reduce", 1003, dtype="f32", op="sum", group="data",
                         quantized=True, ar_algo="ring").destroy()
    L.mlsl_environment_set_quantization_params(
        env, byref(QP(None, None, None, None, 0, 256)))
    d.barrier("global")
    mx.finalize()


def api_errors():
    """ar_algo= where there is no algorithm to name, unknown names, and what
    the C entry point refuses; algo= on an all_reduce still raises."""
    import ctypes
    mx, bufs, rank, size = w._init()
    from mlsl_amd._lib import lib
    from mlsl_amd.api import DTYPE, GROUP, REDOP
    d = mx.Distribution(size, 1)

    def raises(exc, f):
        try:
            f()
        except exc:
            return True
        return False

    def make(kind="all_reduce", **kw):
        kw = dict(dict(dtype="f32", op="sum", group="data", quantized=True), **kw)
        return lambda: mx.PersistentRequest(d, kind, 64, **kw)

    assert raises(ValueError, make(ar_algo="two_shot", quantized=False))
    assert raises(ValueError, make(ar_algo="ring", quantized=False))
    assert raises(ValueError, make("reduce_scatter", ar_algo="two_shot"))
    assert raises(ValueError, make("all_gather", ar_algo="two_shot"))
    assert raises(ValueError, make(ar_algo="tree"))
    assert raises(ValueError, make(ar_algo="direct"))
    assert raises(ValueError, make(algo="direct"))
    assert raises(ValueError, make(algo="ring"))
    # the C entry point: SUM and f32/bf16 only, known algorithms only
    assert raises(RuntimeError, make(ar_algo="two_shot", op="max"))
    assert raises(RuntimeError, make(ar_algo="two_shot", dtype="f64"))
    h = ctypes.c_void_p()
    make(ar_algo="ring")().destroy()   # declares the entry point
    assert lib().mlsl_persistent_all_reduce_quantized_algo(
        d._h, 64, DTYPE["f32"], REDOP["sum"], GROUP["data"], 2, ctypes.byref(h)) != 0
    assert b"unknown" in ctypes.string_at(lib().mlsl_last_error())
    d.barrier("global")
    mx.finalize()


WORKERS = {
    "twoshot_check": twoshot_check,
    "twoshot_error_feedback": twoshot_error_feedback,
    "digest_outputs": digest_outputs,
    "twoshot_too_large": twoshot_too_large,
    "twoshot_plugin": twoshot_plugin,
    "api_errors": api_errors,
}


def main():
    name = sys.argv[1]
    kwargs = json.loads(sys.argv[2]) if len(sys.argv) > 2 else {}
    WORKERS[name](**kwargs)
    print(f"OK {name} rank={os.environ.get('RANK')}")


if __name__ == "__main__":
    main()
