"""Two-shot int8 allreduce on the host: the N-way sum-requantize of
csrc/comm/quant.cpp bit for bit, the schedule, plan and codec under
ASan/UBSan, and the collective over the TCP transport, where the result is
pinned bit for bit at every world size, identical on all ranks, and compared
with the ring.

Expectations, cases and rank workers live in tests/workers_quant_ar.py; the
GPU twin of this file is tests/test_gpu_quant_ar.py.
"""
import os
import subprocess

import numpy as np
import pytest

from tests import quant_ref as qr
from tests import workers_quant_ar as wa
from tests import workers_quant_rs as w
from tests.test_e2e import _run_e2e


# ---- host twin -------------------------------------------------------------

@pytest.mark.parametrize("units,block,nwires", wa.KERNEL_PARAMS)
def test_host_sum_requant_n(units, block, nwires):
    wires = wa.kernel_wires(nwires, units, block)
    got = wa.host_sum_requant_n(wires, units, block)
    assert np.array_equal(got, wa.kernel_expectation(nwires, units, block))


@pytest.mark.parametrize("units,block,nwires,k", wa.ALIAS_PARAMS)
def test_host_sum_requant_n_in_place(units, block, nwires, k):
    # the destination IS wire k: the out-of-place bits, other wires untouched
    wires = wa.kernel_wires(nwires, units, block)
    got = wa.host_sum_requant_n(wires, units, block, alias=k)
    assert np.array_equal(got, wa.kernel_expectation(nwires, units, block))


@pytest.mark.parametrize("block", [128, 256])
def test_host_sum_requant_n_tie_and_zero_blocks(block):
    wa.check_constructed(wa.host_sum_requant_n(wa.constructed_wires(block), 3, block), block)


def test_host_sum_requant_n_one_wire_is_requantize():
    # one wire: the sums are the dequantized values, and quantizing them again
    # is what the pinned codec gives for that input
    units, block = 8, 128
    (wire,) = wa.kernel_wires(1, units, block)
    s, _, q = qr.parse_wire(wire, block)
    v = qr.ref_dequantize(s, q, units * block)
    want = qr.ref_wire(*qr.ref_quantize(v, block))
    assert np.array_equal(wa.host_sum_requant_n([wire], units, block), want)


def test_host_sum_requant_n_order_is_wire_order():
    # 1 + 2^-24 + 2^-24 is 1 when the small terms come last, one at a time,
    # and 1 + 2^-23 when they come first: the block maximum, and with it the
    # new scale, is 1/127 in one order and (1 + 2^-23)/127 in the other
    got = wa.order_case(wa.host_sum_requant_n)
    assert not np.array_equal(got[0], got[1])


def test_host_sum_requant_n_rejects():
    from mlsl_amd import ops
    wires = [np.array(x) for x in wa.kernel_wires(8, 3, 8)]
    dst = np.full(3 * 16, 0xAB, dtype=np.uint8)
    with pytest.raises(RuntimeError, match="1 to 8 wires"):
        ops.host_quant_sum_requant_n([], dst, 3, block=8)
    with pytest.raises(RuntimeError, match="1 to 8 wires"):
        ops.host_quant_sum_requant_n(wires + wires[:1], dst, 3, block=8)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.host_quant_sum_requant_n(wires, dst, 3, block=6)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.host_quant_sum_requant_n(wires, dst, 3, block=0)
    assert (dst == 0xAB).all()


# ---- schedule, plan and codec under ASan/UBSan -----------------------------

def test_quant_ar_twoshot_selftest_asan():
    """Worlds 1 to 9 at 1, 5, 8 and 17 units: slots disjoint and covering
    tmp_bytes, range `to` goes to rank `to`, the gather puts every range in
    its place, one local op; the plan's wire table; worlds 1 to 8:
    HostQuantize -> hand-walked exchange -> HostQuantSumRequantN -> gather ->
    HostDequantize inside plan-sized buffers, equal on all ranks and equal to
    a direct computation."""
    exe = os.path.join(w.REPO, "build", "quant_ar_twoshot_selftest_asan")
    subprocess.run(["make", exe[len(w.REPO) + 1:]], cwd=w.REPO, check=True,
                   capture_output=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS" in r.stdout


# ---- collective, TCP host transport ----------------------------------------

@pytest.mark.parametrize("world", [1, 2, 3, 4, 8])
def test_twoshot_all_reduce(world):
    """Bit for bit against the numpy reference on every rank, f32 and bf16,
    both shapes, in place and out of place; identical on all ranks; at worlds
    3, 4 and 8 also closer to the float64 sum than the ring on the same
    inputs (the ratio is printed by the workers)."""
    outs = wa.run_ranks("twoshot_check", world)
    wa.assert_ranks_agree(outs, world, configs=8)
    for out in outs:
        for line in out.splitlines():
            if line.startswith("rel_l2"):
                print(line)


@pytest.mark.parametrize("world", [2, 3])
def test_twoshot_all_reduce_error_feedback(world):
    wa.run_ranks("twoshot_error_feedback", world)


def test_env_selects_two_shot():
    # MLSL_QUANT_AR_ALGO=two_shot with no ar_algo= is ar_algo="two_shot":
    # the same reference, and the same bits as the named request
    env = wa.run_ranks("twoshot_check", 3, extra_env={"MLSL_QUANT_AR_ALGO": "two_shot"},
                       ar_algo=None, compare_ring=False)
    named = wa.run_ranks("twoshot_check", 3, compare_ring=False)
    assert wa.assert_ranks_agree(env, 3, 8) == wa.assert_ranks_agree(named, 3, 8)


def test_named_ring_ignores_env():
    # ar_algo="ring" under MLSL_QUANT_AR_ALGO=two_shot gives the bits of a
    # plain request without the variable, and those are not two-shot's
    plain = wa.digests(wa.run_ranks("digest_outputs", 3))
    named = wa.digests(wa.run_ranks("digest_outputs", 3, ar_algo="ring",
                                    extra_env={"MLSL_QUANT_AR_ALGO": "two_shot"}))
    two = wa.digests(wa.run_ranks("digest_outputs", 3, ar_algo="two_shot"))
    assert sorted(plain) == [0, 1, 2] and all(len(v) == 8 for v in plain.values())
    assert named == plain
    assert all(a != b for r in plain for a, b in zip(plain[r], two[r]))


def test_env_rejects_unknown_algorithm():
    with pytest.raises(AssertionError, match="expected ring or two_shot"):
        wa.run_ranks("digest_outputs", 1, extra_env={"MLSL_QUANT_AR_ALGO": "tree"})


def test_twoshot_rejects_more_than_8_ranks():
    wa.run_ranks("twoshot_too_large", 9)
    wa.run_ranks("twoshot_too_large", 9, env_choice=True,
                 extra_env={"MLSL_QUANT_AR_ALGO": "two_shot"})


def test_twoshot_rejects_plugin():
    w.ensure_plugin()
    wa.run_ranks("twoshot_plugin", 2)


def test_ar_algo_argument_errors():
    wa.run_ranks("api_errors", 1)


def test_e2e_gradient_requests_follow_the_variable():
    # the runs below would also pass if dl/session.cpp ignored the variable;
    # at 9 ranks they cannot: the ring builds, the two-shot request that a
    # quantized ParameterSet creates is refused with the creation message
    from tests.mp import free_port
    from tests.test_e2e import EXE
    _run_e2e(9, 1, 0, 0, quant=1)
    port = free_port()
    procs = [subprocess.Popen(
        [EXE], cwd=w.REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
        env=dict(os.environ, RANK=str(r), WORLD_SIZE="9", MASTER_ADDR="127.0.0.1",
                 MLSL_PORT=str(port), MLSL_TRANSPORT="tcp", MP="1", DIST_UPDATE="0",
                 USER_BUF="0", QUANT="1", MLSL_QUANT_AR_ALGO="two_shot"))
        for r in range(9)]
    for r, p in enumerate(procs):
        out, _ = p.communicate(timeout=240)
        assert p.returncode != 0 and "PASSED" not in out, f"rank {r}: {out[-1500:]}"
        assert "at most 8 ranks" in out and "MLSL_QUANT_AR_ALGO" in out, \
            f"rank {r}: {out[-3000:]}"


@pytest.mark.parametrize("world,user_buf", [(2, 1), (4, 0)])
def test_e2e_quant_two_shot(world, user_buf):
    # ParameterSet gradients under QUANT=1 follow the variable; mlsl_e2e's own
    # relative-error checks are unchanged
    _run_e2e(world, 1, 0, user_buf, quant=1,
             extra_env={"MLSL_QUANT_AR_ALGO": "two_shot"})
