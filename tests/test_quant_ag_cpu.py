"""int8-quantized all-gather on the host: the segmented dequantize of
csrc/comm/quant.cpp bit for bit, the schedule, plan and codec under
ASan/UBSan, what a request refuses, and the collective over the TCP transport,
where every rank's result is pinned bit for bit at every world size, and
ShardedOptimizer(ag_compression="int8").

Expectations, cases and rank workers live in tests/workers_quant_ag.py; the
GPU twin of this file is tests/test_gpu_quant_ag.py.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import quant_ref as qr
from tests import workers_quant_rs as w
from tests import workers_quant_ag as wa
from tests.mp import free_port


# ---- host twin -------------------------------------------------------------

@pytest.mark.parametrize("count,block,offset,nseg,accumulate,dtype", wa.KERNEL_PARAMS)
def test_host_dequantize_segments(count, block, offset, nseg, accumulate, dtype):
    wire = wa.kernel_wire(nseg, count, block)
    got = wa.host_dequantize_segments(wire, nseg, count, block, dtype, accumulate, offset)
    want = wa.kernel_expectation(nseg, count, block, dtype, accumulate)
    bad = int((got != want).sum())
    assert bad == 0, f"{bad} of {nseg * count} elements differ from the reference"


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("count,block", [(1003, 128), (1280, 256)])
def test_host_assign_is_dequantize_per_segment(count, block, dtype):
    from mlsl_amd import ops
    nseg = 3
    wire = wa.kernel_wire(nseg, count, block)
    got = wa.host_dequantize_segments(wire, nseg, count, block, dtype, False)
    seg_wire = qr.wire_bytes(count, block)
    for j in range(nseg):
        out = np.zeros(count, dtype=w.NP_DT[dtype])
        ops.host_dequantize(np.array(wire[j * seg_wire:(j + 1) * seg_wire]), out, count,
                            block=block, dtype=dtype)
        assert np.array_equal(got[j * count:(j + 1) * count], out.view(w.BITS[dtype])), j


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_host_flat_dequantize_is_wrong_for_partial_blocks(dtype):
    # 1003 = 7 * 128 + 107: segment 1 starts a new block after segment 0's
    # partial one. A flat dequantize of nseg * count elements reads the
    # padding as data instead, and must differ from the expectation.
    from mlsl_amd import ops
    count, block, nseg = 1003, 128, 3
    wire = wa.kernel_wire(nseg, count, block)
    want = wa.kernel_expectation(nseg, count, block, dtype, False)
    flat = np.zeros(nseg * count, dtype=w.NP_DT[dtype])
    ops.host_dequantize(np.array(wire), flat, nseg * count, block=block, dtype=dtype)
    flat = flat.view(w.BITS[dtype])
    assert np.array_equal(flat[:count], want[:count])
    assert (flat[count:] != want[count:]).sum() > count
    got = wa.host_dequantize_segments(wire, nseg, count, block, dtype, False)
    assert np.array_equal(got, want)


def test_host_dequantize_segments_rejects():
    from mlsl_amd import ops
    from mlsl_amd._lib import check, lib
    wire = np.array(wa.kernel_wire(3, 20, 8))
    out = np.full(60, 7.0, dtype=np.float64)
    out32 = np.full(60, 7.0, dtype=np.float32)
    ops.host_dequantize_segments(wire, np.zeros(60, np.float32), 20, 3, block=8)  # declares
    with pytest.raises(RuntimeError, match="f32/bf16 only"):
        check(lib().mlsl_host_dequantize_segments(
            ctypes.c_void_p(wire.ctypes.data), 3, ctypes.c_void_p(out.ctypes.data), 20, 8,
            ops.DTYPE["f64"], 0))
    with pytest.raises(RuntimeError, match="at least one segment"):
        ops.host_dequantize_segments(wire, out32, 20, 0, block=8)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.host_dequantize_segments(wire, out32, 20, 3, block=6)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        check(lib().mlsl_host_dequantize_segments(
            ctypes.c_void_p(wire.ctypes.data), 3, ctypes.c_void_p(out32.ctypes.data), 20, 6,
            ops.DTYPE["f32"], 1))
    assert (out == 7.0).all() and (out32 == 7.0).all(), "a rejected call wrote to out"


# ---- schedule, plan and codec under ASan/UBSan -----------------------------

def test_quant_ag_selftest_asan():
    """Worlds 1 to 9: the simulator accepts the schedules, every segment
    arrives once and in its own place, sends read segment `rank` only; the
    plan's regions; HostQuantize -> hand-walked exchange inside plan-sized
    buffers -> HostDequantizeSegments, assigned and accumulated."""
    exe = os.path.join(w.REPO, "build", "quant_ag_selftest_asan")
    subprocess.run(["make", exe[len(w.REPO) + 1:]], cwd=w.REPO, check=True,
                   capture_output=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS" in r.stdout


def test_request_rejects_all_gatherv_and_f64():
    """The C++ request refuses a compressed all_gatherv and f64 at Setup()
    with errors that name the reason (world 1, no sanitizer)."""
    exe = os.path.join(w.REPO, "build", "quant_ag_request_selftest")
    subprocess.run(["make", exe[len(w.REPO) + 1:]], cwd=w.REPO, check=True,
                   capture_output=True, timeout=600)
    env = dict(os.environ)
    env.update({"RANK": "0", "WORLD_SIZE": "1", "MASTER_ADDR": "127.0.0.1",
                "MLSL_PORT": str(free_port()), "MLSL_TRANSPORT": "tcp"})
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS" in r.stdout


# ---- collective, TCP host transport ----------------------------------------

@pytest.mark.parametrize("world", [1, 2, 3, 4, 8, 9])
def test_quantized_all_gather(world):
    """Bit for bit against the numpy reference on every rank, f32 and bf16,
    both shapes, both modes, out of place and (assign) in place, two starts
    each; one digest across ranks."""
    wa.assert_one_digest(wa.run_ranks("ag_check", world), world)


def test_quantized_all_gather_errors():
    w.ensure_plugin()
    wa.run_ranks("ag_errors", 1)


def test_sharded_optimizer_int8_all_gather():
    wa.run_ranks("ag_sharded_optimizer", 2)


def test_sharded_optimizer_int8_all_gather_with_int8_direct_reduce_scatter():
    wa.run_ranks("ag_sharded_optimizer", 2, compression="int8", rs_algo="direct")
