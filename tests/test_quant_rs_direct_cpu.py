"""One-shot (direct) int8 reduce-scatter on the host: the N-way
sum-dequantize of csrc/comm/quant.cpp bit for bit, the schedule and codec
under ASan/UBSan, and the collective over the TCP transport, where the result
is pinned bit for bit at every world size and compared with the ring.

Expectations, cases and rank workers live in tests/workers_quant_rs_direct.py;
the GPU twin of this file is tests/test_gpu_quant_rs_direct.py.
"""
import os
import subprocess

import numpy as np
import pytest

from tests import quant_ref as qr
from tests import workers_quant_rs as w
from tests import workers_quant_rs_direct as wd


# ---- host twin -------------------------------------------------------------

@pytest.mark.parametrize("count,block,offset,nwires,dtype", wd.KERNEL_PARAMS)
def test_host_sum_dequant_n(count, block, offset, nwires, dtype):
    wires = wd.kernel_wires(nwires, count, block)
    got = wd.host_sum_dequant_n(wires, count, block, dtype, offset)
    assert np.array_equal(got, wd.kernel_expectation(nwires, count, block, dtype))


def test_host_sum_dequant_n_one_wire_is_dequantize():
    # fma(q, s, +0) == q * s: one wire must give the pinned dequantize
    count, block = 1003, 128
    (wire,) = wd.kernel_wires(1, count, block)
    s, _, q = qr.parse_wire(wire, block)
    for dtype in ("f32", "bf16"):
        got = wd.host_sum_dequant_n([wire], count, block, dtype)
        want = qr.ref_dequantize(s, q, count, dtype).view(w.BITS[dtype])
        assert np.array_equal(got, want)


def test_host_sum_dequant_n_order_is_wire_order():
    # three wires whose float32 sum depends on the order of the additions:
    # 1 + 2^-24 + 2^-24 is 1 when the small terms come last, one at a time,
    # and 1 + 2^-23 when they come first
    block = 8
    big = qr.ref_wire(np.array([1.0], np.float32), np.full((1, block), 1, np.int8))
    tiny = qr.ref_wire(np.array([2.0 ** -24], np.float32), np.full((1, block), 1, np.int8))
    one = np.float32(1.0).view(np.uint32)
    assert (wd.host_sum_dequant_n([big, tiny, tiny], block, block, "f32") == one).all()
    assert (wd.host_sum_dequant_n([tiny, tiny, big], block, block, "f32") == one + 1).all()


def test_host_sum_dequant_n_rejects():
    from mlsl_amd import ops
    from mlsl_amd._lib import check, lib
    import ctypes
    wires = list(wd.kernel_wires(8, 20, 8))
    out = np.zeros(20, dtype=np.float64)
    ops.host_quant_sum_dequant_n(wires, out.view(np.float32), 20, block=8)  # declares
    ptrs = (ctypes.c_void_p * 8)(*[x.ctypes.data for x in wires])
    with pytest.raises(RuntimeError, match="f32/bf16 only"):
        check(lib().mlsl_host_quant_sum_dequant_n(ptrs, 8, out.ctypes.data, 20, 8,
                                                  ops.DTYPE["f64"]))
    with pytest.raises(RuntimeError, match="1 to 8 wires"):
        ops.host_quant_sum_dequant_n([], out.view(np.float32), 20, block=8)
    with pytest.raises(RuntimeError, match="1 to 8 wires"):
        ops.host_quant_sum_dequant_n(wires + wires[:1], out.view(np.float32), 20, block=8)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.host_quant_sum_dequant_n(wires, out.view(np.float32), 20, block=6)


# ---- schedule and codec under ASan/UBSan -----------------------------------

def test_quant_rs_direct_selftest_asan():
    """Worlds 1 to 9: the simulator accepts the schedules, the receive slots
    are disjoint and cover tmp_bytes, segment `to` goes to rank `to`; worlds
    2 to 8: HostQuantize -> hand-walked exchange -> HostQuantSumDequantN."""
    exe = os.path.join(w.REPO, "build", "quant_rs_direct_selftest_asan")
    subprocess.run(["make", exe[len(w.REPO) + 1:]], cwd=w.REPO, check=True,
                   capture_output=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS" in r.stdout


# ---- collective, TCP host transport ----------------------------------------

@pytest.mark.parametrize("world", [1, 2, 3, 4, 8])
def test_direct_reduce_scatter(world):
    """Bit for bit against the numpy reference on every rank, f32 and bf16,
    both shapes, in place and out of place; from world 3 up also closer to
    the float64 sum than the ring on the same inputs."""
    wd.run_ranks("direct_check", world)


def test_direct_reduce_scatter_error_feedback():
    wd.run_ranks("direct_error_feedback", 3)


def test_env_selects_direct():
    # MLSL_QUANT_RS_ALGO=direct with no algo= is algo="direct": same reference
    wd.run_ranks("direct_check", 3, extra_env={"MLSL_QUANT_RS_ALGO": "direct"},
                 algo=None, compare_ring=False)


def test_named_ring_ignores_env():
    # algo="ring" under MLSL_QUANT_RS_ALGO=direct gives the bits of a ring
    # request (no algo=) without the variable, and those are not direct's
    plain = wd.digests(wd.run_ranks("digest_outputs", 3))
    named = wd.digests(wd.run_ranks("digest_outputs", 3, algo="ring",
                                    extra_env={"MLSL_QUANT_RS_ALGO": "direct"}))
    direct = wd.digests(wd.run_ranks("digest_outputs", 3, algo="direct"))
    assert sorted(plain) == [0, 1, 2] and all(len(v) == 8 for v in plain.values())
    assert named == plain
    assert all(a != b for r in plain for a, b in zip(plain[r], direct[r]))


def test_direct_rejects_more_than_8_ranks():
    wd.run_ranks("direct_too_large", 9)


def test_direct_rejects_plugin():
    w.ensure_plugin()
    wd.run_ranks("direct_plugin", 2)


def test_algo_argument_errors():
    wd.run_ranks("api_errors", 1)


def test_sharded_optimizer_int8_direct():
    wd.run_ranks("direct_sharded_optimizer", 2)
