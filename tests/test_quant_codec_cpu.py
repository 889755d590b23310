"""Host int8 codec (csrc/comm/quant.cpp) against the numpy reference in
tests/quant_ref.py, bit for bit, and the rejection of unsupported block
sizes. No GPU: the host entry points take numpy arrays.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import quant_ref as qr

# the codec shapes of tests/test_gpu_kernels_exact.py that are not there
# only to reach a GPU dispatch arm: fewer elements per block than lanes;
# a tail block with scalar tail and padding at 128, 256 and 512; whole
# blocks with an odd block count
SHAPES = [(20, 8), (1003, 128), (1000, 256), (5000, 512), (1280, 256)]
NP_DT = {"f32": np.float32, "bf16": np.uint16}


def _ops():
    from mlsl_amd import ops
    return ops


def _guards_intact(*wholes):
    return all((w[-qr.GUARD:] == 0xCD).all() for w in wholes)


@pytest.mark.parametrize("use_err", [True, False], ids=["err", "noerr"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("count,block", SHAPES)
def test_host_codec_matches_reference(count, block, dtype, use_err):
    ops = _ops()
    inp, err0 = qr.make_input(count, block, dtype, seed=count + block)
    want = qr.codec_expectation(inp, err0 if use_err else None, count, block, dtype)

    wire_w, wire = qr.guarded(qr.wire_bytes(count, block), np.uint8, 0xAB)
    out_w, out = qr.guarded(count, NP_DT[dtype], 0xAB)
    err_w, err = qr.guarded(count, NP_DT[dtype], 0)
    err[:] = err0
    inp_before = inp.copy()

    ops.host_quantize(inp, wire, count, err=err if use_err else None, block=block,
                      dtype=dtype)
    ops.host_dequantize(wire, out, count, block=block, dtype=dtype)

    assert np.array_equal(wire, want["wire"])
    assert np.array_equal(out.view(np.uint8), want["out"].view(np.uint8))
    if use_err:
        # x86-64 host code has no fused multiply-add here
        assert np.array_equal(err.view(np.uint8), want["err_unfused"].view(np.uint8))
    else:
        assert np.array_equal(err, err0)
    assert np.array_equal(inp, inp_before)
    assert _guards_intact(wire_w, out_w, err_w)
    # the special blocks, spelled out
    scales, word1, q = qr.parse_wire(wire, block)
    assert scales[qr.TIE_BLOCK] == np.float32(0.125) and scales[qr.ZERO_BLOCK] == 1.0
    assert not word1.view(np.uint32).any()
    assert not q[qr.ZERO_BLOCK].any()
    tie = qr.decode(inp, dtype)[:block] * np.float32(8)
    assert (q[qr.TIE_BLOCK][1:] % 2 == 0).all()          # ties go to even
    assert (np.abs(q[qr.TIE_BLOCK] - tie) <= 0.5).all()  # ... the nearest ones


@pytest.mark.parametrize("count,block", [(1280, 256), (1000, 256), (1003, 128), (20, 8)])
def test_host_quant_accum_exact_wires(count, block):
    ops = _ops()
    a, b, want = qr.make_exact_wires(count, block, seed=count)
    acc_w, acc = qr.guarded(a.size, np.uint8, 0)
    acc[:] = a
    b_before = b.copy()
    ops.host_quant_accum(acc, b, count, block=block)
    assert np.array_equal(acc, want)
    assert np.array_equal(b, b_before)
    assert _guards_intact(acc_w)


@pytest.mark.parametrize("count,block", [(1 << 14, 256), (10003, 128)])
def test_host_quant_accum_random_wires(count, block):
    # wires of quantized random data: the host evaluates a*as + b*bs with
    # two roundings, which numpy float32 reproduces
    ops = _ops()
    rng = np.random.default_rng(count)
    wires = []
    for mul in (1.0, 7.0):
        v = (rng.standard_normal(count) * mul).astype(np.float32)
        w = np.empty(qr.wire_bytes(count, block), dtype=np.uint8)
        ops.host_quantize(v, w, count, block=block)
        assert np.array_equal(w, qr.ref_wire(*qr.ref_quantize(v, block)))
        wires.append(w)
    want = qr.ref_quant_accum_unfused(wires[0], wires[1], count, block)
    ops.host_quant_accum(wires[0], wires[1], count, block=block)
    assert np.array_equal(wires[0], want)


def test_reference_candidates_differ():
    # the two residual forms are really two: a test that accepted only one
    # of them would be wrong about fused code
    v, _ = qr.make_input(5000, 256, "f32", seed=1)
    scales, q = qr.ref_quantize(v, 256)
    r0, r1 = qr.ref_residuals(v, scales, q)
    assert (r0 != r1).mean() > 0.25
    assert np.abs(r0.astype(np.float64) - r1).max() < 1e-6


# ---- unsupported block sizes ----------------------------------------------

BAD_BLOCKS = [0, 1, 6, 254, 258]


@pytest.mark.parametrize("block", BAD_BLOCKS)
def test_host_wrappers_reject_block(block):
    ops = _ops()
    buf = np.zeros(4096, dtype=np.uint8)
    f = np.zeros(16, dtype=np.float32)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.host_quantize(f, buf, 16, block=block)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.host_dequantize(buf, f, 16, block=block)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.host_quant_accum(buf, buf.copy(), 16, block=block)


@pytest.mark.parametrize("block", BAD_BLOCKS)
def test_c_entry_points_reject_block(block):
    """Host ops and device launchers fail before they touch a buffer (or
    launch anything): the buffers here are host memory and stay as they are."""
    ops = _ops()
    from mlsl_amd._lib import MlslError, check
    L = ops._lib()
    buf = np.full(4096, 0x5A, dtype=np.uint8)
    p = ctypes.c_void_p(buf.__array_interface__["data"][0])
    calls = [
        lambda: L.mlsl_host_quantize(p, p, p, 16, block, 0, 1),
        lambda: L.mlsl_host_dequantize(p, p, 16, block, 0),
        lambda: L.mlsl_host_quant_accum(p, p, 16, block),
        lambda: L.mlsl_hip_quantize(p, p, p, 16, block, 0, 1),
        lambda: L.mlsl_hip_dequantize(p, p, 16, block, 0),
        lambda: L.mlsl_hip_dequantize_nt(p, p, 16, block, 0),
        lambda: L.mlsl_hip_quantize_f32_nt(p, p, p, 16, block),
        lambda: L.mlsl_hip_quant_accum(p, p, 16, block),
    ]
    for call in calls:
        with pytest.raises(MlslError, match="block"):
            check(call())
    assert (buf == 0x5A).all()


@pytest.mark.parametrize("block", BAD_BLOCKS)
def test_set_quant_params_rejects_block(block):
    import mlsl_amd as mx
    from mlsl_amd._lib import MlslError, lib
    got = ctypes.c_size_t(0)
    lib().mlsl_get_quant_params.argtypes = [ctypes.POINTER(ctypes.c_size_t)]
    lib().mlsl_get_quant_params(ctypes.byref(got))
    before = got.value
    with pytest.raises(MlslError, match="multiple of 4"):
        mx.set_quant_params(block)
    lib().mlsl_get_quant_params(ctypes.byref(got))
    assert got.value == before


class _QuantParams(ctypes.Structure):
    _fields_ = [("lib_path", ctypes.c_char_p),
                ("quant_buffer_func_name", ctypes.c_char_p),
                ("dequant_buffer_func_name", ctypes.c_char_p),
                ("reduce_sum_func_name", ctypes.c_char_p),
                ("block_size", ctypes.c_size_t), ("elem_in_block", ctypes.c_size_t)]


def test_environment_quant_params_reject_block():
    from mlsl_amd._lib import lib
    L = lib()
    fn = L.mlsl_environment_set_quantization_params
    fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(_QuantParams)]
    fn.restype = ctypes.c_int
    for block in BAD_BLOCKS:
        qp = _QuantParams(None, None, None, None, 0, block)
        assert fn(None, ctypes.byref(qp)) != 0
        assert b"block" in L.mlsl_last_error() or b"elem_in_block" in L.mlsl_last_error()
    for block in (128, 256):
        qp = _QuantParams(None, None, None, None, 0, block)
        assert fn(None, ctypes.byref(qp)) == 0, L.mlsl_last_error()
    # a plugin library defines its own wire block: its elem_in_block is not
    # the built-in codec's business
    qp = _QuantParams(b"/nonexistent/libplugin.so", None, None, None, 70, 62)
    assert fn(None, ctypes.byref(qp)) == 0, L.mlsl_last_error()
    qp = _QuantParams(None, None, None, None, 0, 256)
    assert fn(None, ctypes.byref(qp)) == 0


@pytest.mark.parametrize("block,ok", [("6", False), ("0", False), ("128", True)])
def test_env_quant_block(block, ok):
    code = ("import mlsl_amd as mx\n"
            "try:\n"
            "    mx.init()\n"
            "except Exception as e:\n"
            "    print('REJECTED', e)\n"
            "else:\n"
            "    mx.finalize(); print('ACCEPTED')\n")
    env = dict(os.environ, MLSL_QUANT_BLOCK=block, MLSL_TRANSPORT="tcp")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    if ok:
        assert "ACCEPTED" in r.stdout
    else:
        assert "REJECTED" in r.stdout and "MLSL_QUANT_BLOCK" in r.stdout
