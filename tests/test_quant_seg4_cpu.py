"""The int4 allreduce over a list of tensors on the CPU: the host twins of the
gather and scatter kernels against tests/quant4_ref.py on the concatenation,
bit for bit; SegmentedAllReduce(compression="int4") over TCP against the flat
bits=4 request; DistributedData(compression="int4"); the sanitizer self-test."""
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import workers_quant_rs as wrs  # noqa: E402
from tests import workers_quant_seg4 as w4  # noqa: E402
from tests.mp import REPO  # noqa: E402


@pytest.mark.parametrize("case", [p for p in w4.PARAMS if p[5] is None] + w4.TRIP_PARAMS,
                         ids=str)
def test_host_twins(case):
    w4.run_codec_case(w4.HostApi(), *case)


def test_host_rejects():
    from mlsl_amd import ops
    a, wire = np.zeros(8, np.float32), np.zeros(64, np.uint8)
    for f, args in ((ops.host_quantize_gather4, ([a, a], [8, 8], wire)),
                    (ops.host_dequantize_scatter4, (wire, [a, a], [8, 8]))):
        with pytest.raises(ValueError, match="multiple of 8 at 4 bits"):
            f(*args, block=12)
        with pytest.raises(ValueError, match="f32/bf16 only"):
            f(*args, block=8, dtype="f64")
    with pytest.raises(ValueError, match="at least one segment"):
        ops.host_quantize_gather4([], [], wire, block=8)
    with pytest.raises(ValueError, match="at least one element"):
        ops.host_dequantize_scatter4(wire, [a, a], [8, 0], block=8)


@pytest.mark.parametrize("world", [1, 2, 3, 4, 8])
def test_request_matches_flat_bits4(world):
    w4.run_ranks("seg4_check", world)


@pytest.mark.parametrize("world,plugin", [(2, True), (9, False)])
def test_request_refusals(world, plugin):
    if plugin:
        wrs.ensure_plugin()
    w4.run_ranks("seg4_refusals", world, plugin=plugin)


@pytest.mark.parametrize("with_f64", [False, True])
def test_ddp_int4_matches_flat_requests(with_f64):
    w4.run_ranks("ddp4_check", 2, with_f64=with_f64)


def test_sanitizer_selftest():
    """csrc/tests/quant_seg4_selftest.cpp under ASan/UBSan, as an executable."""
    exe = os.path.join("build", "quant_seg4_selftest_asan")
    subprocess.run(["make", exe], cwd=REPO, check=True, capture_output=True, timeout=600)
    r = subprocess.run([os.path.join(REPO, exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "quant_seg4_selftest: all passed" in r.stdout, \
        (r.stdout + r.stderr)[-4000:]
