"""The quantized allreduce over a list of tensors on the CPU: the host twins
of the gather and scatter kernels against the numpy reference, bit for bit;
the request over TCP against the flat quantized request on the materialised
concatenation; DistributedData(compression="int8"); the sanitizer self-test.
"""
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import quant_seg_ref as sr  # noqa: E402
from tests import workers_quant_rs as wrs  # noqa: E402
from tests import workers_quant_seg as ws  # noqa: E402
from tests.mp import REPO  # noqa: E402


class TestHostTwins:
    @pytest.mark.parametrize("case", ws.CODEC_PARAMS, ids=ws.codec_id)
    def test_against_numpy(self, case):
        ws.run_codec_case(ws.HostApi(), *case)

    def test_two_roundings_differ_from_one(self):
        # the reference itself: (q * scale) * f32(1/3) is not q * (scale *
        # f32(1/3)) everywhere, and is the same thing at 1.0 and 0.5
        want = sr.gather_expectation("edges", 256, "f32", True)
        n = sum(sr.LAYOUTS["edges"])
        for ps, differs in ((1.0, False), (0.5, False), (1.0 / 3.0, True)):
            two = sr.ref_dequantize_scatter(want["wire"], n, 256, "f32", ps)
            one = sr.ref_dequantize_fused_scale(want["wire"], n, 256, "f32", ps)
            assert bool((two.view(np.uint32) != one.view(np.uint32)).any()) == differs

    def test_rejects(self):
        from mlsl_amd import ops
        from mlsl_amd._lib import MlslError
        a, b = np.zeros(8, np.float32), np.zeros(8, np.float32)
        wire = np.zeros(sr.qr.wire_bytes(16, 8), np.uint8)
        with pytest.raises(ValueError, match="at least one element"):
            ops.host_quantize_gather([a, b], [8, 0], wire, block=8)
        with pytest.raises(ValueError, match="at least one segment"):
            ops.host_quantize_gather([], [], wire, block=8)
        with pytest.raises(ValueError, match="f32/bf16 only"):
            ops.host_quantize_gather([a, b], [8, 8], wire, block=8, dtype="f64")
        with pytest.raises(ValueError, match="multiple of 4"):
            ops.host_quantize_gather([a, b], [8, 8], wire, block=6)
        with pytest.raises(ValueError, match="at least one element"):
            ops.host_dequantize_scatter(wire, [a, b], [0, 8], block=8)
        with pytest.raises(ValueError, match="at least one segment"):
            ops.host_dequantize_scatter(wire, [], [], block=8)
        with pytest.raises(ValueError, match="f32/bf16 only"):
            ops.host_dequantize_scatter(wire, [a, b], [8, 8], block=8, dtype="f16")
        with pytest.raises(ValueError, match="multiple of 4"):
            ops.host_dequantize_scatter(wire, [a, b], [8, 8], block=0)
        with pytest.raises(ValueError, match="counts"):
            ops.host_quantize_gather([a], [8, 8], wire, block=8)
        # the C entry points refuse the same things on their own
        import ctypes
        L = ops._lib()
        ptrs = (ctypes.c_void_p * 2)(a.ctypes.data, b.ctypes.data)
        wp = ctypes.c_void_p(wire.ctypes.data)
        for counts, nseg, block, dt, needle in (
                ([8, 0], 2, 8, 0, "segment 1 is empty"), ([8, 8], 0, 8, 0, "at least one"),
                ([8, 8], 2, 8, 1, "f32/bf16 only"), ([8, 8], 2, 6, 0, "multiple of 4")):
            cnt = (ctypes.c_size_t * 2)(*counts)
            assert L.mlsl_host_quantize_gather(ptrs, cnt, nseg, None, wp, block, dt, 0) != 0
            assert needle in ctypes.string_at(L.mlsl_last_error()).decode()
            assert L.mlsl_host_dequantize_scatter(wp, ptrs, cnt, nseg, block, dt, 1.0, 0) != 0
            assert needle in ctypes.string_at(L.mlsl_last_error()).decode()
        assert issubclass(MlslError, RuntimeError)


class TestCollectiveTcp:
    # post_scale 1 and 1/world; at world 1 they are the same case
    @pytest.mark.parametrize(
        "world,algo,dtype,inv_world",
        [(n, a, t, inv) for n in (1, 2, 3, 4, 8) for a in ("ring", "two_shot")
         for t in ("f32", "bf16") for inv in ((False, True) if n > 1 else (False,))],
        ids=lambda v: {True: "psinv", False: "ps1"}.get(v, str(v)) if isinstance(v, bool)
        else str(v))
    def test_matches_flat_request(self, world, algo, dtype, inv_world):
        """World 3 with 1/world is the case that tells the request's rounding
        apart: for bf16 the finish rounds q * scale to bf16 before it scales
        (round_first), as the flat request followed by a multiplication
        does; one rounding after the scaling differs there in a quarter of
        the elements."""
        outs = ws.run_ranks("seg_check", world, algos=[algo], dtypes=[dtype],
                            inv_world=inv_world)
        ws.assert_ranks_agree(outs, world)

    @pytest.mark.parametrize("env_algo", ["two_shot", "ring"])
    def test_env_algo_honoured(self, env_algo):
        ws.run_ranks("seg_env_algo", 3, extra_env={"MLSL_QUANT_AR_ALGO": env_algo},
                     env_algo=env_algo)

    @pytest.mark.parametrize("world", [1, 2])
    def test_refusals(self, world):
        ws.run_ranks("seg_refusals", world)

    def test_two_shot_refused_past_8_ranks(self):
        ws.run_ranks("seg_refusals", 9)

    def test_plugin_refused(self):
        wrs.ensure_plugin()
        ws.run_ranks("seg_plugin", 2)


class TestDdpTcp:
    def test_int8_matches_flat_requests(self):
        outs = ws.run_ranks("ddp_check", 2)
        ws.assert_ranks_agree(outs, 2)

    def test_f64_bucket_stays_exact(self):
        outs = ws.run_ranks("ddp_check", 2, with_f64=True)
        ws.assert_ranks_agree(outs, 2)

    def test_keywords(self):
        from mlsl_amd.parallel import DistributedData
        m = torch.nn.Linear(2, 2)
        with pytest.raises(ValueError, match="compression"):
            DistributedData(m, dist=object(), compression="fp8")
        with pytest.raises(ValueError, match="ar_algo"):
            DistributedData(m, dist=object(), ar_algo="ring")


def test_sanitizer_selftest():
    """csrc/tests/quant_seg_selftest.cpp under ASan/UBSan: the host twins over
    exact-size heap tensors, and the hand-walked exchange at worlds 1 to 9."""
    exe = os.path.join(REPO, "build", "quant_seg_selftest_asan")
    subprocess.run(["make", exe[len(REPO) + 1:]], cwd=REPO, check=True,
                   capture_output=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "quant_seg_selftest: all passed" in r.stdout, r.stdout[-2000:]
