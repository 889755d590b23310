"""The quantized reduce-scatter over a list of tensors on the CPU: the host
twin of the prologue kernel against the numpy reference and the flat host
quantize, bit for bit; the request over TCP against the flat quantized
reduce_scatter on the materialised, padded concatenation;
ShardedOptimizer(grads="in_place") against grads="copy"; the sanitizer
self-test.
"""
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import quant_seg_ref as sr  # noqa: E402
from tests import workers_quant_rs as wrs  # noqa: E402
from tests import workers_quant_rs_seg as wq  # noqa: E402
from tests.mp import REPO  # noqa: E402


class TestHostTwin:
    @pytest.mark.parametrize("case", wq.SHARD_PARAMS, ids=wq.shard_id)
    def test_against_numpy_and_flat(self, case):
        wq.run_shard_case(wq.HostApi(), *case)

    @pytest.mark.parametrize("dtype", ["f32", "bf16"])
    @pytest.mark.parametrize("case", wq.ODD_WIRE_SHARD_CASES, ids=str)
    def test_wire_of_4_mod_8_bytes(self, case, dtype):
        # blocks of 12 and 100 elements, an odd number per shard: the plan's
        # stride, one shard's wire exactly, is a multiple of 4 and not of 8
        layout, n, shard, block = case
        sw = sr.qr.wire_bytes(shard, block)
        assert sw % 8 == 4
        for misalign in (False, True):
            wq.run_shard_case(wq.HostApi(), layout, n, shard, block, dtype, True, misalign,
                              wire_stride=sw)

    @pytest.mark.parametrize("extra", [0, 4, 8, 24])
    def test_wire_stride(self, extra):
        # the plan's stride is one shard's wire exactly
        stride = sr.qr.wire_bytes(513, 256) + extra
        wq.run_shard_case(wq.HostApi(), "edges", 4, 513, 256, "f32", True, True,
                          wire_stride=stride)

    def test_rejects(self):
        from mlsl_amd import ops
        a, b = np.zeros(8, np.float32), np.zeros(8, np.float32)
        wire = np.zeros(2 * sr.qr.wire_bytes(8, 8), np.uint8)
        f = ops.host_quantize_gather_shards
        with pytest.raises(ValueError, match="at least one element"):
            f([a, b], [8, 0], wire, 2, 8, block=8)
        with pytest.raises(ValueError, match="at least one segment"):
            f([], [], wire, 2, 8, block=8)
        with pytest.raises(ValueError, match=r"shard \* nshards < total"):
            f([a, b], [8, 8], wire, 2, 7, block=8)
        with pytest.raises(ValueError, match=r"shard \* nshards < total"):
            f([a, b], [8, 8], wire, 0, 8, block=8)
        with pytest.raises(ValueError, match="f32/bf16 only"):
            f([a, b], [8, 8], wire, 2, 8, block=8, dtype="f64")
        with pytest.raises(ValueError, match="multiple of 4"):
            f([a, b], [8, 8], wire, 2, 8, block=6)
        with pytest.raises(ValueError, match="wire_stride"):
            f([a, b], [8, 8], wire, 2, 8, block=8, wire_stride=8)
        with pytest.raises(ValueError, match="wire_stride"):
            f([a, b], [8, 8], wire, 2, 8, block=8, wire_stride=18)
        # the C entry point refuses the same things on its own
        import ctypes
        L = ops._lib()
        ptrs = (ctypes.c_void_p * 2)(a.ctypes.data, b.ctypes.data)
        wp = ctypes.c_void_p(wire.ctypes.data)
        for counts, nseg, nshards, shard, stride, block, dt, needle in (
                ([8, 0], 2, 2, 8, 16, 8, 0, "segment 1 is empty"),
                ([8, 8], 0, 2, 8, 16, 8, 0, "at least one"),
                ([8, 8], 2, 2, 7, 16, 8, 0, "shard * nshards < total"),
                ([8, 8], 2, 0, 8, 16, 8, 0, "shard * nshards < total"),
                ([8, 8], 2, 2, 8, 8, 8, 0, "wire_stride"),
                ([8, 8], 2, 2, 8, 16, 8, 1, "f32/bf16 only"),
                ([8, 8], 2, 2, 8, 16, 6, 0, "multiple of 4")):
            cnt = (ctypes.c_size_t * 2)(*counts)
            assert L.mlsl_host_quantize_gather_shards(ptrs, cnt, nseg, None, wp, nshards, shard,
                                                      stride, block, dt, 0) != 0
            assert needle in ctypes.string_at(L.mlsl_last_error()).decode()
        assert not wire.any() and not a.any() and not b.any(), "a rejected call wrote"


class TestCollectiveTcp:
    @pytest.mark.parametrize("dtype", ["f32", "bf16"])
    @pytest.mark.parametrize("algo", ["ring", "direct"])
    @pytest.mark.parametrize("world", [1, 2, 3, 4, 8])
    def test_matches_flat_request(self, world, algo, dtype):
        """edges, about 3 MiB of ragged tensors, five elements (at worlds 4
        and 8 some ranks own nothing but padding) and a shard larger than it
        has to be; three starts each, the residual carried."""
        outs = wq.run_ranks("rs_seg_check", world, algos=[algo], dtypes=[dtype])
        wq.assert_all_checked(outs, world)

    @pytest.mark.parametrize("algo", ["ring", "direct"])
    @pytest.mark.parametrize("world", [1, 2, 3, 4])
    def test_block_of_12_matches_flat_request(self, world, algo):
        """A wire block of 20 bytes: the plan's seg_wire is 4 (mod 8) for the
        24-element list at every world, as it may be for any supported block."""
        outs = wq.run_ranks("rs_seg_check", world, algos=[algo], block=wq.ODD_WIRE_BLOCK)
        wq.assert_all_checked(outs, world)

    @pytest.mark.parametrize("env_algo", ["direct", "ring"])
    def test_env_algo_honoured(self, env_algo):
        wq.run_ranks("rs_seg_env_algo", 3, extra_env={"MLSL_QUANT_RS_ALGO": env_algo},
                     env_algo=env_algo)

    @pytest.mark.parametrize("world", [1, 2])
    def test_refusals(self, world):
        wq.run_ranks("rs_seg_refusals", world)

    def test_direct_refused_past_8_ranks(self):
        wq.run_ranks("rs_seg_refusals", 9)

    def test_plugin_refused(self):
        wrs.ensure_plugin()
        wq.run_ranks("rs_seg_plugin", 2)


class TestShardedOptimizerTcp:
    @pytest.mark.parametrize("rs_algo,ag", [("ring", "none"), ("direct", "none"),
                                            ("ring", "int8")])
    def test_in_place_matches_copy(self, rs_algo, ag):
        outs = wq.run_ranks("zero1_check", 2, rs_algo=rs_algo, ag_compression=ag)
        wq.assert_all_checked(outs, 2)

    @pytest.mark.parametrize("world", [1, 2])
    def test_refusals(self, world):
        wq.run_ranks("zero1_refusals", world)


def test_sanitizer_selftest():
    """csrc/tests/quant_rs_seg_selftest.cpp under ASan/UBSan: the host twin
    over exact-size heap tensors, and the hand-walked exchanges at worlds 1 to
    9."""
    exe = os.path.join(REPO, "build", "quant_rs_seg_selftest_asan")
    subprocess.run(["make", exe[len(REPO) + 1:]], cwd=REPO, check=True,
                   capture_output=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "quant_rs_seg_selftest: all passed" in r.stdout, r.stdout[-2000:]
