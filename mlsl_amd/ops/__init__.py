"""Standalone CDNA4 kernel ops (device-pointer API over the HIP kernels in
csrc/hip/kernels.hip): local reductions, int8 block quantization with error
feedback, and pack/unpack. Used by GPU numerics tests and by consumers that
want the fused kernels without the full Session machinery.

Buffers: torch CUDA tensors, raw integer device pointers, or anything with
``data_ptr()``. The ``host_*`` functions run the host codec of
csrc/comm/quant.cpp (same wire format) on numpy arrays.
"""
import ctypes
import math

from .._lib import lib as _core_lib, check
from ..api import DTYPE, REDOP, _as_ptr_dtype

_declared = False


def _lib():
    global _declared
    L = _core_lib()
    if not _declared:
        c = ctypes
        L.mlsl_hip_device_count.argtypes = [c.POINTER(c.c_int)]
        L.mlsl_hip_synchronize.argtypes = []
        L.mlsl_hip_reduce.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t, c.c_int, c.c_int]
        L.mlsl_hip_reduce_nt.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t]
        L.mlsl_hip_copy.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t]
        L.mlsl_hip_reduce_nt2.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t]
        L.mlsl_hip_copy_variant.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t, c.c_int]
        L.mlsl_hip_quantize.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t,
                                        c.c_size_t, c.c_int, c.c_int]
        L.mlsl_hip_dequantize.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t,
                                          c.c_size_t, c.c_int]
        L.mlsl_hip_dequantize_nt.argtypes = L.mlsl_hip_dequantize.argtypes
        L.mlsl_hip_quantize_f32_nt.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p,
                                               c.c_size_t, c.c_size_t]
        L.mlsl_hip_quant_accum.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t, c.c_size_t]
        L.mlsl_hip_quant_sum_dequant.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p,
                                                 c.c_size_t, c.c_size_t, c.c_int]
        L.mlsl_hip_quant_sum_dequant_nt.argtypes = L.mlsl_hip_quant_sum_dequant.argtypes
        L.mlsl_host_quant_sum_dequant.argtypes = L.mlsl_hip_quant_sum_dequant.argtypes
        L.mlsl_hip_quant_sum_dequant_n.argtypes = [c.POINTER(c.c_void_p), c.c_int,
                                                   c.c_void_p, c.c_size_t, c.c_size_t,
                                                   c.c_int]
        L.mlsl_host_quant_sum_dequant_n.argtypes = L.mlsl_hip_quant_sum_dequant_n.argtypes
        L.mlsl_hip_quant_sum_requant_n.argtypes = [c.POINTER(c.c_void_p), c.c_int,
                                                   c.c_void_p, c.c_size_t, c.c_size_t]
        L.mlsl_host_quant_sum_requant_n.argtypes = L.mlsl_hip_quant_sum_requant_n.argtypes
        L.mlsl_hip_quant_sum_requant_n.restype = c.c_int
        L.mlsl_host_quant_sum_requant_n.restype = c.c_int
        L.mlsl_hip_quantize4.argtypes = L.mlsl_hip_quantize.argtypes + [c.c_int]
        L.mlsl_hip_dequantize4.argtypes = L.mlsl_hip_dequantize.argtypes + [c.c_int]
        L.mlsl_hip_quant_sum_dequant_n4.argtypes = \
            L.mlsl_hip_quant_sum_dequant_n.argtypes + [c.c_int]
        L.mlsl_hip_quant_sum_requant_n4.argtypes = \
            L.mlsl_hip_quant_sum_requant_n.argtypes + [c.c_int]
        L.mlsl_hip_quant4_blocks_per_trip.argtypes = [c.c_int, c.POINTER(c.c_size_t)]
        L.mlsl_host_quantize4.argtypes = L.mlsl_hip_quantize.argtypes
        L.mlsl_host_dequantize4.argtypes = L.mlsl_hip_dequantize.argtypes
        L.mlsl_host_quant_sum_dequant_n4.argtypes = L.mlsl_hip_quant_sum_dequant_n.argtypes
        L.mlsl_host_quant_sum_requant_n4.argtypes = L.mlsl_hip_quant_sum_requant_n.argtypes
        for n in ("quantize4", "dequantize4", "quant_sum_dequant_n4", "quant_sum_requant_n4"):
            getattr(L, "mlsl_hip_" + n).restype = c.c_int
            getattr(L, "mlsl_host_" + n).restype = c.c_int
        L.mlsl_hip_quant4_blocks_per_trip.restype = c.c_int
        L.mlsl_hip_dequantize_segments.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p,
                                                   c.c_size_t, c.c_size_t, c.c_int, c.c_int]
        L.mlsl_host_dequantize_segments.argtypes = L.mlsl_hip_dequantize_segments.argtypes
        L.mlsl_hip_dequantize_segments.restype = c.c_int
        L.mlsl_host_dequantize_segments.restype = c.c_int
        L.mlsl_hip_dequantize_segments4.argtypes = \
            L.mlsl_hip_dequantize_segments.argtypes + [c.c_int]
        L.mlsl_host_dequantize_segments4.argtypes = L.mlsl_hip_dequantize_segments.argtypes
        L.mlsl_hip_dequantize_segments4.restype = c.c_int
        L.mlsl_host_dequantize_segments4.restype = c.c_int
        L.mlsl_hip_quantize_gather.argtypes = [c.POINTER(c.c_void_p),
                                               c.POINTER(c.c_size_t), c.c_size_t,
                                               c.c_void_p, c.c_void_p, c.c_size_t,
                                               c.c_int, c.c_int]
        L.mlsl_host_quantize_gather.argtypes = L.mlsl_hip_quantize_gather.argtypes
        L.mlsl_hip_dequantize_scatter.argtypes = [c.c_void_p, c.POINTER(c.c_void_p),
                                                  c.POINTER(c.c_size_t), c.c_size_t,
                                                  c.c_size_t, c.c_int, c.c_float,
                                                  c.c_int]
        L.mlsl_host_dequantize_scatter.argtypes = L.mlsl_hip_dequantize_scatter.argtypes
        L.mlsl_hip_quantize_gather_tables.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t,
                                                      c.c_void_p, c.c_void_p, c.c_size_t,
                                                      c.c_size_t, c.c_int, c.c_int]
        L.mlsl_hip_dequantize_scatter_tables.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p,
                                                         c.c_size_t, c.c_size_t, c.c_size_t,
                                                         c.c_int, c.c_float, c.c_int]
        L.mlsl_hip_quantize_gather4.argtypes = L.mlsl_hip_quantize_gather.argtypes + [c.c_int]
        L.mlsl_hip_dequantize_scatter4.argtypes = \
            L.mlsl_hip_dequantize_scatter.argtypes + [c.c_int]
        L.mlsl_hip_quantize_gather4_tables.argtypes = \
            L.mlsl_hip_quantize_gather_tables.argtypes + [c.c_int]
        L.mlsl_hip_dequantize_scatter4_tables.argtypes = \
            L.mlsl_hip_dequantize_scatter_tables.argtypes + [c.c_int]
        L.mlsl_host_quantize_gather4.argtypes = L.mlsl_hip_quantize_gather.argtypes
        L.mlsl_host_dequantize_scatter4.argtypes = L.mlsl_hip_dequantize_scatter.argtypes
        for n in ("mlsl_hip_quantize_gather4", "mlsl_hip_dequantize_scatter4",
                  "mlsl_hip_quantize_gather4_tables", "mlsl_hip_dequantize_scatter4_tables",
                  "mlsl_host_quantize_gather4", "mlsl_host_dequantize_scatter4"):
            getattr(L, n).restype = c.c_int
        L.mlsl_hip_gather_list.argtypes = [c.POINTER(c.c_void_p), c.POINTER(c.c_size_t),
                                           c.c_size_t, c.c_void_p, c.c_int]
        L.mlsl_host_gather_list.argtypes = L.mlsl_hip_gather_list.argtypes
        L.mlsl_hip_scatter_scale_list.argtypes = [c.c_void_p, c.POINTER(c.c_void_p),
                                                  c.POINTER(c.c_size_t), c.c_size_t, c.c_int,
                                                  c.c_float]
        L.mlsl_host_scatter_scale_list.argtypes = L.mlsl_hip_scatter_scale_list.argtypes
        L.mlsl_hip_gather_list_tables.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t,
                                                  c.c_void_p, c.c_size_t, c.c_int]
        L.mlsl_hip_scatter_scale_list_tables.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p,
                                                         c.c_size_t, c.c_size_t, c.c_int,
                                                         c.c_float]
        L.mlsl_hip_list_elems_per_trip.argtypes = [c.c_int, c.POINTER(c.c_size_t)]
        for n in ("mlsl_hip_gather_list", "mlsl_host_gather_list",
                  "mlsl_hip_scatter_scale_list", "mlsl_host_scatter_scale_list",
                  "mlsl_hip_gather_list_tables", "mlsl_hip_scatter_scale_list_tables",
                  "mlsl_hip_list_elems_per_trip"):
            getattr(L, n).restype = c.c_int
        L.mlsl_hip_sumsq.argtypes = [c.c_void_p, c.c_size_t, c.c_int, c.c_void_p, c.c_int]
        L.mlsl_hip_sumsq_list.argtypes = [c.POINTER(c.c_void_p), c.POINTER(c.c_size_t),
                                          c.c_size_t, c.c_int, c.c_void_p, c.c_int]
        L.mlsl_hip_sumsq_list_tables.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t,
                                                 c.c_size_t, c.c_int, c.c_void_p, c.c_int]
        L.mlsl_hip_clip_scale.argtypes = [c.c_void_p, c.c_size_t, c.c_int, c.c_void_p,
                                          c.c_float]
        L.mlsl_hip_clip_scale_list.argtypes = [c.POINTER(c.c_void_p), c.POINTER(c.c_size_t),
                                               c.c_size_t, c.c_int, c.c_void_p, c.c_float]
        L.mlsl_hip_clip_scale_list_tables.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t,
                                                      c.c_size_t, c.c_int, c.c_void_p,
                                                      c.c_float]
        for n in ("mlsl_hip_sumsq", "mlsl_hip_sumsq_list", "mlsl_hip_sumsq_list_tables",
                  "mlsl_hip_clip_scale", "mlsl_hip_clip_scale_list",
                  "mlsl_hip_clip_scale_list_tables"):
            getattr(L, n).restype = c.c_int
        L.mlsl_hip_adamw_step.argtypes = [c.c_void_p] * 6 + [c.c_size_t, c.c_int, c.c_void_p,
                                                              c.POINTER(c.c_float), c.c_int]
        L.mlsl_host_adamw_step.argtypes = L.mlsl_hip_adamw_step.argtypes[:-1]
        L.mlsl_hip_adamw_elems_per_trip.argtypes = [c.POINTER(c.c_size_t)]
        for n in ("mlsl_hip_adamw_step", "mlsl_host_adamw_step",
                  "mlsl_hip_adamw_elems_per_trip"):
            getattr(L, n).restype = c.c_int
        L.mlsl_hip_quantize_gather_tables.restype = c.c_int
        L.mlsl_hip_dequantize_scatter_tables.restype = c.c_int
        L.mlsl_hip_quantize_gather_shards.argtypes = [c.POINTER(c.c_void_p),
                                                      c.POINTER(c.c_size_t), c.c_size_t,
                                                      c.c_void_p, c.c_void_p, c.c_size_t,
                                                      c.c_size_t, c.c_size_t, c.c_size_t,
                                                      c.c_int, c.c_int]
        L.mlsl_host_quantize_gather_shards.argtypes = \
            L.mlsl_hip_quantize_gather_shards.argtypes
        L.mlsl_hip_quantize_gather_shards_tables.argtypes = [
            c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p, c.c_size_t,
            c.c_size_t, c.c_size_t, c.c_size_t, c.c_size_t, c.c_int, c.c_int]
        L.mlsl_hip_quantize_gather_shards4.argtypes = \
            L.mlsl_hip_quantize_gather_shards.argtypes + [c.c_int]
        L.mlsl_hip_quantize_gather_shards4_tables.argtypes = \
            L.mlsl_hip_quantize_gather_shards_tables.argtypes + [c.c_int]
        L.mlsl_host_quantize_gather_shards4.argtypes = \
            L.mlsl_hip_quantize_gather_shards.argtypes
        for n in ("mlsl_hip_quantize_gather_shards", "mlsl_host_quantize_gather_shards",
                  "mlsl_hip_quantize_gather_shards_tables",
                  "mlsl_hip_quantize_gather_shards4", "mlsl_host_quantize_gather_shards4",
                  "mlsl_hip_quantize_gather_shards4_tables"):
            getattr(L, n).restype = c.c_int
        for n in ("mlsl_hip_quantize_gather", "mlsl_host_quantize_gather",
                  "mlsl_hip_dequantize_scatter", "mlsl_host_dequantize_scatter"):
            getattr(L, n).restype = c.c_int
        L.mlsl_host_quantize.argtypes = L.mlsl_hip_quantize.argtypes
        L.mlsl_host_dequantize.argtypes = L.mlsl_hip_dequantize.argtypes
        L.mlsl_host_quant_accum.argtypes = L.mlsl_hip_quant_accum.argtypes
        for n in ("mlsl_host_quantize", "mlsl_host_dequantize", "mlsl_host_quant_accum",
                  "mlsl_hip_quant_sum_dequant", "mlsl_hip_quant_sum_dequant_nt",
                  "mlsl_host_quant_sum_dequant", "mlsl_hip_quant_sum_dequant_n",
                  "mlsl_host_quant_sum_dequant_n"):
            getattr(L, n).restype = c.c_int
        ptypes = [c.c_void_p, c.c_void_p] + [c.c_size_t] * 8 + [c.c_int]
        L.mlsl_hip_pack.argtypes = ptypes
        L.mlsl_hip_unpack.argtypes = ptypes
        for n in ("mlsl_hip_device_count", "mlsl_hip_synchronize", "mlsl_hip_reduce",
                  "mlsl_hip_reduce_nt", "mlsl_hip_reduce_nt2", "mlsl_hip_copy", "mlsl_hip_copy_variant",
                  "mlsl_hip_quantize", "mlsl_hip_dequantize", "mlsl_hip_dequantize_nt", "mlsl_hip_quantize_f32_nt", "mlsl_hip_quant_accum",
                  "mlsl_hip_pack", "mlsl_hip_unpack"):
            getattr(L, n).restype = c.c_int
        _declared = True
    return L


def device_count():
    n = ctypes.c_int(0)
    _lib().mlsl_hip_device_count(ctypes.byref(n))
    return n.value


def synchronize():
    check(_lib().mlsl_hip_synchronize())


def reduce_(dst, src, count, dtype=None, op="sum"):
    """dst op= src on device (count elements)."""
    dp, d1 = _as_ptr_dtype(dst)
    sp, d2 = _as_ptr_dtype(src)
    dt = dtype or d1 or d2
    check(_lib().mlsl_hip_reduce(dp, sp, count, DTYPE[dt], REDOP[op]))


def reduce_nt(dst, src, count):
    """f32 sum with nontemporal loads/stores (benchmark variant)."""
    dp, _ = _as_ptr_dtype(dst)
    sp, _ = _as_ptr_dtype(src)
    check(_lib().mlsl_hip_reduce_nt(dp, sp, count))


def reduce_nt2(dst, src, count):
    dp, _ = _as_ptr_dtype(dst)
    sp, _ = _as_ptr_dtype(src)
    check(_lib().mlsl_hip_reduce_nt2(dp, sp, count))


def copy(dst, src, bytes_):
    """Streaming D2D copy (NT kernel for large aligned transfers)."""
    dp, _ = _as_ptr_dtype(dst)
    sp, _ = _as_ptr_dtype(src)
    check(_lib().mlsl_hip_copy(dp, sp, bytes_))


def copy_variant(dst, src, bytes_, nt):
    dp, _ = _as_ptr_dtype(dst)
    sp, _ = _as_ptr_dtype(src)
    check(_lib().mlsl_hip_copy_variant(dp, sp, bytes_, 1 if nt else 0))


def wire_bytes(count, block=256, bits=8):
    """Bytes of the wire format for `count` elements: int8 (bits=8) or int4
    (bits=4) payload after each block's 8-byte header."""
    nblocks = (count + block - 1) // block
    return nblocks * (block * bits // 8 + 8)


_PATH4 = {None: 0, "generic": 1, "fast": 2}


def _check_block4(block):
    if block == 0 or block % 8:
        raise ValueError(f"quantization block of {block} elements is not supported "
                         "(must be a non-zero multiple of 8 at 4 bits)")


def quant4_blocks_per_trip(fast):
    """Wire blocks one launch of an int4 kernel covers before its grid-stride
    loop takes a second trip, on the fast or the generic path."""
    n = ctypes.c_size_t(0)
    check(_lib().mlsl_hip_quant4_blocks_per_trip(1 if fast else 0, ctypes.byref(n)))
    return n.value


def quantize4(inp, wire, count, err=None, block=256, dtype=None, path=None):
    """`quantize` into the int4 wire: [f32 scale][f32 0][block/2 bytes] per
    block, element i in nibble i & 1 of payload byte i >> 1, scale = max/7,
    q in -7..7; `err`, if given, is added to the input and left holding the
    residual fma(-q, scale, v). block is a multiple of 8. path=None lets the
    launcher choose its kernel, "generic" or "fast" names it (the A/B hook;
    "fast" needs block 256, whole blocks and aligned buffers)."""
    _check_block4(block)
    ip, d1 = _as_ptr_dtype(inp)
    wp, _ = _as_ptr_dtype(wire)
    ep, _ = _as_ptr_dtype(err)
    check(_lib().mlsl_hip_quantize4(ip, ep, wp, count, block, DTYPE[dtype or d1],
                                    1 if err is not None else 0, _PATH4[path]))


def dequantize4(wire, out, count, block=256, dtype=None, path=None):
    """`dequantize` of an int4 wire (see `quantize4`)."""
    _check_block4(block)
    wp, _ = _as_ptr_dtype(wire)
    op_, d1 = _as_ptr_dtype(out)
    check(_lib().mlsl_hip_dequantize4(wp, op_, count, block, DTYPE[dtype or d1],
                                      _PATH4[path]))


def quant_sum_dequant_n4(wires, out, count, block=256, dtype=None, path=None):
    """`quant_sum_dequant_n` over int4 wires: the finish of the direct
    reduce_scatter at bits=4."""
    _check_block4(block)
    ptrs = (ctypes.c_void_p * len(wires))(*[_as_ptr_dtype(w)[0].value for w in wires])
    op_, d1 = _as_ptr_dtype(out)
    check(_lib().mlsl_hip_quant_sum_dequant_n4(ptrs, len(wires), op_, count, block,
                                               DTYPE[dtype or d1], _PATH4[path]))


def quant_sum_requant_n4(wires, dst, nunits, block=256, path=None):
    """`quant_sum_requant_n` over int4 wires, units of block/2 + 8 bytes: the
    owner's step of the two-shot all_reduce at bits=4. `dst` may be exactly
    one of the wires or overlap none."""
    _check_block4(block)
    ptrs = (ctypes.c_void_p * len(wires))(*[_as_ptr_dtype(w)[0].value for w in wires])
    dp, _ = _as_ptr_dtype(dst)
    check(_lib().mlsl_hip_quant_sum_requant_n4(ptrs, len(wires), dp, nunits, block,
                                               _PATH4[path]))


def quantize(inp, wire, count, err=None, block=256, dtype=None):
    ip, d1 = _as_ptr_dtype(inp)
    wp, _ = _as_ptr_dtype(wire)
    ep, _ = _as_ptr_dtype(err)
    dt = dtype or d1
    check(_lib().mlsl_hip_quantize(ip, ep, wp, count, block, DTYPE[dt],
                                   1 if err is not None else 0))


def dequantize(wire, out, count, block=256, dtype=None):
    wp, _ = _as_ptr_dtype(wire)
    op_, d1 = _as_ptr_dtype(out)
    dt = dtype or d1
    check(_lib().mlsl_hip_dequantize(wp, op_, count, block, DTYPE[dt]))


def quantize_f32_nt(inp, wire, count, err, block=256):
    ip, _ = _as_ptr_dtype(inp)
    wp, _ = _as_ptr_dtype(wire)
    ep, _ = _as_ptr_dtype(err)
    check(_lib().mlsl_hip_quantize_f32_nt(ip, ep, wp, count, block))


def dequantize_nt(wire, out, count, block=256, dtype=None):
    wp, _ = _as_ptr_dtype(wire)
    op_, d1 = _as_ptr_dtype(out)
    dt = dtype or d1
    check(_lib().mlsl_hip_dequantize_nt(wp, op_, count, block, DTYPE[dt]))


def quant_accum(acc_wire, wire, count, block=256):
    ap, _ = _as_ptr_dtype(acc_wire)
    wp, _ = _as_ptr_dtype(wire)
    check(_lib().mlsl_hip_quant_accum(ap, wp, count, block))


def quant_sum_dequant(a_wire, b_wire, out, count, block=256, dtype=None):
    """out = dequantize(a_wire) + dequantize(b_wire) in one pass, in the
    element type of `out` (f32/bf16); the wires are not written. The last hop
    of the quantized reduce-scatter, which never requantizes the sum."""
    ap, _ = _as_ptr_dtype(a_wire)
    bp, _ = _as_ptr_dtype(b_wire)
    op_, d1 = _as_ptr_dtype(out)
    dt = dtype or d1
    check(_lib().mlsl_hip_quant_sum_dequant(ap, bp, op_, count, block, DTYPE[dt]))


def quant_sum_dequant_nt(a_wire, b_wire, out, count, block=256, dtype=None):
    """`quant_sum_dequant` with nontemporal stores (benchmark variant)."""
    ap, _ = _as_ptr_dtype(a_wire)
    bp, _ = _as_ptr_dtype(b_wire)
    op_, d1 = _as_ptr_dtype(out)
    dt = dtype or d1
    check(_lib().mlsl_hip_quant_sum_dequant_nt(ap, bp, op_, count, block, DTYPE[dt]))


def quant_sum_dequant_n(wires, out, count, block=256, dtype=None):
    """out = the sum of dequantize(w) over the 1 to 8 `wires`, in one pass and
    in the element type of `out` (f32/bf16); no wire is written. Per element
    the sum starts at +0 and takes one fma per wire, in the order given: the
    fan-in of the one-shot quantized reduce-scatter (algo="direct")."""
    ptrs = (ctypes.c_void_p * len(wires))(*[_as_ptr_dtype(w)[0].value for w in wires])
    op_, d1 = _as_ptr_dtype(out)
    dt = dtype or d1
    check(_lib().mlsl_hip_quant_sum_dequant_n(ptrs, len(wires), op_, count, block,
                                              DTYPE[dt]))


def quant_sum_requant_n(wires, dst, nunits, block=256):
    """dst = requantize(the sum of dequantize(w) over the 1 to 8 `wires`), over
    `nunits` whole wire units of block + 8 bytes: no element count and no
    dtype. Per element the sum starts at +0 and takes one fma per wire, in the
    order given; each block is requantized once, with `quantize`'s codec.
    `dst` may be exactly one of the wires (the sum replaces it in place) or
    overlap none of them. The owner's step of the two-shot quantized
    all_reduce (ar_algo="two_shot")."""
    ptrs = (ctypes.c_void_p * len(wires))(*[_as_ptr_dtype(w)[0].value for w in wires])
    dp, _ = _as_ptr_dtype(dst)
    check(_lib().mlsl_hip_quant_sum_requant_n(ptrs, len(wires), dp, nunits, block))


def dequantize_segments(wire, out, count, nseg, block=256, dtype=None, accumulate=False):
    """The finish of the quantized all_gather in one launch: `wire` holds
    `nseg` segment wires of wire_bytes(count, block) bytes, each on a block
    grid of its own, and segment j goes to out[j*count:(j+1)*count] (f32/bf16).
    Assigned with the bits of `dequantize`, or with accumulate=True as
    out = fma(q, scale, out) in float, rounded once. Any nseg >= 1; the wire
    is not written."""
    wp, _ = _as_ptr_dtype(wire)
    op_, d1 = _as_ptr_dtype(out)
    dt = dtype or d1
    check(_lib().mlsl_hip_dequantize_segments(wp, nseg, op_, count, block, DTYPE[dt],
                                              1 if accumulate else 0))


def dequantize_segments4(wire, out, count, nseg, block=256, dtype=None, accumulate=False,
                         path=None):
    """`dequantize_segments` of int4 wires, the finish of the all_gather at
    bits=4: `wire` holds `nseg` segment wires of wire_bytes(count, block, 4)
    bytes back to back, 4-byte aligned, and segment j goes to
    out[j*count:(j+1)*count] (f32/bf16) as q * scale, or with accumulate=True
    as fma(q, scale, out) in float, rounded once. `out` and count may have any
    alignment. path as in `quantize4`: "fast" needs block 256, count a multiple
    of 256, `out` 16-byte and the wire 8-byte aligned; None takes it wherever
    it fits."""
    _check_block4(block)
    wp, _ = _as_ptr_dtype(wire)
    op_, d1 = _as_ptr_dtype(out)
    check(_lib().mlsl_hip_dequantize_segments4(wp, nseg, op_, count, block,
                                               DTYPE[dtype or d1], 1 if accumulate else 0,
                                               _PATH4[path]))


def _seg_tables(tensors, counts, dtype):
    """(pointer array, count array, nseg, total, dtype name) of a list of
    tensors: device tensors, raw pointers or anything _as_ptr_dtype takes."""
    if len(tensors) != len(counts):
        raise ValueError(f"{len(tensors)} tensors but {len(counts)} counts")
    if not counts:
        raise ValueError("the tensor list is empty: at least one segment is needed")
    for j, n in enumerate(counts):
        if int(n) < 1:
            raise ValueError(f"counts[{j}] = {n}: every segment needs at least one element")
    pd = [_as_ptr_dtype(t) for t in tensors]
    ptrs = (ctypes.c_void_p * len(pd))(*[p.value for p, _ in pd])
    return (ptrs, (ctypes.c_size_t * len(counts))(*[int(n) for n in counts]), len(counts),
            sum(int(n) for n in counts), dtype or pd[0][1])


def quantize_gather(tensors, counts, wire, err=None, block=256, dtype=None):
    """`quantize` of the concatenation of `tensors` (counts[j] elements each,
    f32/bf16) without materialising it: `wire`, and the flat residual `err` of
    sum(counts) elements if given, get exactly the bytes `quantize` writes for
    torch.cat(tensors). The tensors are only read; their addresses need the
    element's alignment only, and boundaries fall anywhere in a wire block.
    The segment tables are uploaded here, once per call."""
    _check_block(block)
    ptrs, cnts, nseg, _, dt = _seg_tables(tensors, counts, dtype)
    wp, _ = _as_ptr_dtype(wire)
    ep, _ = _as_ptr_dtype(err)
    check(_lib().mlsl_hip_quantize_gather(ptrs, cnts, nseg, ep, wp, block, DTYPE[dt],
                                          1 if err is not None else 0))


def dequantize_scatter(wire, tensors, counts, block=256, dtype=None, post_scale=1.0,
                       round_first=False):
    """`dequantize` of `wire` into the list `tensors`, scaled: element i of
    tensor j becomes (q * scale) * post_scale, both products rounded to
    float32 (two roundings, never one product with scale * post_scale) and
    bf16 rounded once more. post_scale=1.0 gives `dequantize`'s bits. The wire
    is only read and nothing outside the tensors is written.
    round_first=True (bf16; f32 does not change) rounds q * scale to bf16
    before it is scaled: the bits of `dequantize` followed by a float32
    multiplication of the stored elements, which is what the request over a
    tensor list (SegmentedAllReduce) computes."""
    _check_block(block)
    ptrs, cnts, nseg, _, dt = _seg_tables(tensors, counts, dtype)
    wp, _ = _as_ptr_dtype(wire)
    check(_lib().mlsl_hip_dequantize_scatter(wp, ptrs, cnts, nseg, block, DTYPE[dt],
                                             post_scale, 1 if round_first else 0))


def quantize_gather4(tensors, counts, wire, err=None, block=256, dtype=None, path=None):
    """`quantize_gather` into the int4 wire: exactly the bytes `quantize4`
    writes for torch.cat(tensors), in `wire` and, if given, in the flat
    residual `err` (one fma(-q, scale, v), pinned bit for bit). block is a
    multiple of 8 and the wire 4-byte aligned. path=None takes one block per
    half-wave at block 256 and one wave per block otherwise; "generic" or
    "fast" names it ("fast" needs block 256)."""
    _check_block4(block)
    ptrs, cnts, nseg, _, dt = _seg_tables(tensors, counts, dtype)
    wp, _ = _as_ptr_dtype(wire)
    ep, _ = _as_ptr_dtype(err)
    check(_lib().mlsl_hip_quantize_gather4(ptrs, cnts, nseg, ep, wp, block, DTYPE[dt],
                                           1 if err is not None else 0, _PATH4[path]))


def dequantize_scatter4(wire, tensors, counts, block=256, dtype=None, post_scale=1.0,
                        round_first=False, path=None):
    """`dequantize_scatter` of an int4 wire: (q * scale) * post_scale with
    both products rounded to float32; post_scale=1.0 gives `dequantize4`'s
    bits. round_first and path as in `dequantize_scatter` and
    `quantize_gather4`."""
    _check_block4(block)
    ptrs, cnts, nseg, _, dt = _seg_tables(tensors, counts, dtype)
    wp, _ = _as_ptr_dtype(wire)
    check(_lib().mlsl_hip_dequantize_scatter4(wp, ptrs, cnts, nseg, block, DTYPE[dt],
                                              post_scale, 1 if round_first else 0,
                                              _PATH4[path]))


def quantize_gather4_tables(dev_ptrs, dev_offs, nseg, count, wire, err=None, block=256,
                            dtype="f32", path=None):
    """`quantize_gather4` over tables in DEVICE memory; see
    `quantize_gather_tables`."""
    _check_block4(block)
    pp, _ = _as_ptr_dtype(dev_ptrs)
    fp, _ = _as_ptr_dtype(dev_offs)
    wp, _ = _as_ptr_dtype(wire)
    ep, _ = _as_ptr_dtype(err)
    check(_lib().mlsl_hip_quantize_gather4_tables(pp, fp, nseg, ep, wp, count, block,
                                                  DTYPE[dtype], 1 if err is not None else 0,
                                                  _PATH4[path]))


def dequantize_scatter4_tables(wire, dev_ptrs, dev_offs, nseg, count, block=256, dtype="f32",
                               post_scale=1.0, round_first=False, path=None):
    """`dequantize_scatter4` over tables in DEVICE memory; see
    `quantize_gather_tables`."""
    _check_block4(block)
    pp, _ = _as_ptr_dtype(dev_ptrs)
    fp, _ = _as_ptr_dtype(dev_offs)
    wp, _ = _as_ptr_dtype(wire)
    check(_lib().mlsl_hip_dequantize_scatter4_tables(wp, pp, fp, nseg, count, block,
                                                     DTYPE[dtype], post_scale,
                                                     1 if round_first else 0, _PATH4[path]))


def _shard_args(total, nshards, shard, wire_stride, block, bits=8):
    """(nshards, shard, wire_stride) checked; wire_stride=None is one shard's
    wire bytes rounded up to 16."""
    nshards, shard = int(nshards), int(shard)
    if nshards < 1 or shard * nshards < total:
        raise ValueError(f"shard * nshards < total: {nshards} shards of {shard} elements "
                         f"do not hold {total}")
    need = wire_bytes(shard, block, bits)
    if wire_stride is None:
        wire_stride = (need + 15) // 16 * 16
    wire_stride = int(wire_stride)
    if wire_stride < need or wire_stride % 4:
        raise ValueError(f"wire_stride={wire_stride}: a multiple of 4 of at least {need} "
                         "bytes (one shard's wire) is needed")
    return nshards, shard, wire_stride


def quantize_gather_shards(tensors, counts, wire, nshards, shard, err=None, block=256,
                           dtype=None, wire_stride=None):
    """`quantize_gather` shard by shard, in one launch: with V' the
    concatenation of `tensors` followed by zeros up to nshards * shard
    elements (never built), shard j = V'[j*shard:(j+1)*shard] gets exactly the
    bytes `quantize` writes for it, at wire + j * wire_stride, and the residual
    `err` (if given: nshards * shard elements, flat in V' order) at err + j *
    shard. wire_stride=None is wire_bytes(shard, block) rounded up to 16; the
    bytes between two shards' wires are left alone. A shard may begin or end
    inside a tensor or be padding only. A padding element quantizes as 0, is
    read through no pointer, and its residual (+0 from the start) is neither
    read nor written. This is the prologue of `SegmentedReduceScatter`."""
    _check_block(block)
    ptrs, cnts, nseg, total, dt = _seg_tables(tensors, counts, dtype)
    nshards, shard, wire_stride = _shard_args(total, nshards, shard, wire_stride, block)
    wp, _ = _as_ptr_dtype(wire)
    ep, _ = _as_ptr_dtype(err)
    check(_lib().mlsl_hip_quantize_gather_shards(ptrs, cnts, nseg, ep, wp, nshards, shard,
                                                 wire_stride, block, DTYPE[dt],
                                                 1 if err is not None else 0))


def quantize_gather_shards_tables(dev_ptrs, dev_offs, nseg, total, wire, nshards, shard,
                                  err=None, block=256, dtype="f32", wire_stride=None):
    """`quantize_gather_shards` over tables in DEVICE memory; see
    `quantize_gather_tables` (dev_offs runs from 0 to total)."""
    _check_block(block)
    nshards, shard, wire_stride = _shard_args(total, nshards, shard, wire_stride, block)
    pp, _ = _as_ptr_dtype(dev_ptrs)
    fp, _ = _as_ptr_dtype(dev_offs)
    wp, _ = _as_ptr_dtype(wire)
    ep, _ = _as_ptr_dtype(err)
    check(_lib().mlsl_hip_quantize_gather_shards_tables(
        pp, fp, nseg, ep, wp, total, nshards, shard, wire_stride, block, DTYPE[dtype],
        1 if err is not None else 0))


def quantize_gather_shards4(tensors, counts, wire, nshards, shard, err=None, block=256,
                            dtype=None, wire_stride=None, path=None):
    """`quantize_gather_shards` into the int4 wire, in one launch: shard j of
    V' gets exactly the bytes `quantize4` writes for it, at wire + j *
    wire_stride, and the residual (one fma(-q, scale, v), pinned bit for bit)
    at err + j * shard. block is a multiple of 8, the wire 4-byte aligned,
    wire_stride=None is wire_bytes(shard, block, 4) rounded up to 16. Padding
    as in `quantize_gather_shards`: the value 0, read through no pointer, its
    residual left alone. path as in `quantize_gather4`; at "fast" the two
    blocks of a half-wave pair may lie in different shards. This is the
    prologue of `SegmentedReduceScatter(compression="int4")`."""
    _check_block4(block)
    ptrs, cnts, nseg, total, dt = _seg_tables(tensors, counts, dtype)
    nshards, shard, wire_stride = _shard_args(total, nshards, shard, wire_stride, block, 4)
    wp, _ = _as_ptr_dtype(wire)
    ep, _ = _as_ptr_dtype(err)
    check(_lib().mlsl_hip_quantize_gather_shards4(ptrs, cnts, nseg, ep, wp, nshards, shard,
                                                  wire_stride, block, DTYPE[dt],
                                                  1 if err is not None else 0, _PATH4[path]))


def quantize_gather_shards4_tables(dev_ptrs, dev_offs, nseg, total, wire, nshards, shard,
                                   err=None, block=256, dtype="f32", wire_stride=None,
                                   path=None):
    """`quantize_gather_shards4` over tables in DEVICE memory; see
    `quantize_gather_tables` (dev_offs runs from 0 to total)."""
    _check_block4(block)
    nshards, shard, wire_stride = _shard_args(total, nshards, shard, wire_stride, block, 4)
    pp, _ = _as_ptr_dtype(dev_ptrs)
    fp, _ = _as_ptr_dtype(dev_offs)
    wp, _ = _as_ptr_dtype(wire)
    ep, _ = _as_ptr_dtype(err)
    check(_lib().mlsl_hip_quantize_gather_shards4_tables(
        pp, fp, nseg, ep, wp, total, nshards, shard, wire_stride, block, DTYPE[dtype],
        1 if err is not None else 0, _PATH4[path]))


def quantize_gather_tables(dev_ptrs, dev_offs, nseg, count, wire, err=None, block=256,
                           dtype="f32"):
    """`quantize_gather` over tables the caller keeps in DEVICE memory, as a
    request does: dev_offs holds nseg + 1 prefix offsets (64-bit, from 0 to
    count), dev_ptrs the nseg tensor addresses (64-bit). Nothing is uploaded
    and nothing about the tables can be checked here."""
    _check_block(block)
    pp, _ = _as_ptr_dtype(dev_ptrs)
    fp, _ = _as_ptr_dtype(dev_offs)
    wp, _ = _as_ptr_dtype(wire)
    ep, _ = _as_ptr_dtype(err)
    check(_lib().mlsl_hip_quantize_gather_tables(pp, fp, nseg, ep, wp, count, block,
                                                 DTYPE[dtype], 1 if err is not None else 0))


def dequantize_scatter_tables(wire, dev_ptrs, dev_offs, nseg, count, block=256, dtype="f32",
                              post_scale=1.0, round_first=False):
    """`dequantize_scatter` over tables in DEVICE memory; see
    `quantize_gather_tables`."""
    _check_block(block)
    pp, _ = _as_ptr_dtype(dev_ptrs)
    fp, _ = _as_ptr_dtype(dev_offs)
    wp, _ = _as_ptr_dtype(wire)
    check(_lib().mlsl_hip_dequantize_scatter_tables(wp, pp, fp, nseg, count, block,
                                                    DTYPE[dtype], post_scale,
                                                    1 if round_first else 0))


def gather_list(tensors, counts, flat, dtype=None):
    """torch.cat(tensors) into `flat` in one launch, as raw bits (f32, bf16 or
    f16; NaN payloads and -0 survive): `flat`, 16-byte aligned, gets sum(counts)
    elements and nothing past them. The tensors (counts[j] elements each) are
    only read and need their element's alignment only."""
    ptrs, cnts, nseg, _, dt = _seg_tables(tensors, counts, dtype)
    fp, _ = _as_ptr_dtype(flat)
    check(_lib().mlsl_hip_gather_list(ptrs, cnts, nseg, fp, DTYPE[dt]))


def scatter_scale_list(flat, tensors, counts, dtype=None, post_scale=1.0):
    """`flat` back into the list `tensors`, scaled: element i of the
    concatenation becomes flat[i] * post_scale, one float32 product rounded once
    into the element type; post_scale=1.0 copies the bits. `flat` is only read
    and nothing outside the tensors is written."""
    ptrs, cnts, nseg, _, dt = _seg_tables(tensors, counts, dtype)
    fp, _ = _as_ptr_dtype(flat)
    check(_lib().mlsl_hip_scatter_scale_list(fp, ptrs, cnts, nseg, DTYPE[dt], post_scale))


def gather_list_tables(dev_ptrs, dev_offs, nseg, count, flat, dtype="f32"):
    """`gather_list` over tables in DEVICE memory; see `quantize_gather_tables`."""
    pp, _ = _as_ptr_dtype(dev_ptrs)
    op_, _ = _as_ptr_dtype(dev_offs)
    fp, _ = _as_ptr_dtype(flat)
    check(_lib().mlsl_hip_gather_list_tables(pp, op_, nseg, fp, count, DTYPE[dtype]))


def scatter_scale_list_tables(flat, dev_ptrs, dev_offs, nseg, count, dtype="f32",
                              post_scale=1.0):
    """`scatter_scale_list` over tables in DEVICE memory; see
    `quantize_gather_tables`."""
    pp, _ = _as_ptr_dtype(dev_ptrs)
    op_, _ = _as_ptr_dtype(dev_offs)
    fp, _ = _as_ptr_dtype(flat)
    check(_lib().mlsl_hip_scatter_scale_list_tables(fp, pp, op_, nseg, count, DTYPE[dtype],
                                                    post_scale))


def list_elems_per_trip(dtype):
    """Elements one launch of `gather_list`, `scatter_scale_list`, `sumsq`,
    `sumsq_list`, `clip_scale` or `clip_scale_list` covers before its
    grid-stride loop takes a second trip."""
    n = ctypes.c_size_t(0)
    check(_lib().mlsl_hip_list_elems_per_trip(DTYPE[dtype], ctypes.byref(n)))
    return n.value


def _f64_scalar(t, what):
    """Pointer of the device f64 scalar `t`: a 1-element torch.float64 tensor or
    a raw pointer."""
    p, dt = _as_ptr_dtype(t)
    if dt is not None and (dt != "f64" or t.numel() != 1):
        raise ValueError(f"{what} must be one float64 element in device memory, not "
                         f"{t.numel()} of {t.dtype}")
    return p


def sumsq(inp, count, out, dtype=None, accumulate=False):
    """out = (out if accumulate else 0) + the sum of the squares of the first
    `count` elements of `inp` (f32, bf16 or f16), every element converted to
    float64 first and everything added in float64. `out` is a device f64
    scalar: a 1-element torch.float64 tensor or a raw pointer; it is never read
    back here. No atomics: the same input at the same address modulo 16 gives
    the same bits every time."""
    ip, d1 = _as_ptr_dtype(inp)
    check(_lib().mlsl_hip_sumsq(ip, count, DTYPE[dtype or d1], _f64_scalar(out, "out"),
                                1 if accumulate else 0))


def sumsq_list(tensors, counts, out, dtype=None, accumulate=False):
    """`sumsq` of the concatenation of `tensors` (counts[j] elements each) in
    one launch, without building it. The segment tables are uploaded here, once
    per call."""
    ptrs, cnts, nseg, _, dt = _seg_tables(tensors, counts, dtype)
    check(_lib().mlsl_hip_sumsq_list(ptrs, cnts, nseg, DTYPE[dt], _f64_scalar(out, "out"),
                                     1 if accumulate else 0))


def sumsq_list_tables(dev_ptrs, dev_offs, nseg, count, out, dtype="f32", accumulate=False):
    """`sumsq_list` over tables in DEVICE memory; see `quantize_gather_tables`."""
    pp, _ = _as_ptr_dtype(dev_ptrs)
    op_, _ = _as_ptr_dtype(dev_offs)
    check(_lib().mlsl_hip_sumsq_list_tables(pp, op_, nseg, count, DTYPE[dtype],
                                            _f64_scalar(out, "out"), 1 if accumulate else 0))


def clip_scale(data, count, total, max_norm, dtype=None):
    """Gradient clipping's scale, in place: the first `count` elements of `data`
    times float32(min(1, max_norm / (sqrt(total) + 1e-6))), torch's coefficient,
    one float32 product rounded once into the element type. `total`, the squared
    norm, is a device f64 scalar as `sumsq` leaves it; the kernel reads it, the
    host does not. max_norm is taken as a float32."""
    dp, d1 = _as_ptr_dtype(data)
    check(_lib().mlsl_hip_clip_scale(dp, count, DTYPE[dtype or d1],
                                     _f64_scalar(total, "total"), max_norm))


def clip_scale_list(tensors, counts, total, max_norm, dtype=None):
    """`clip_scale` of every tensor of the list in one launch; nothing outside
    the tensors is written. The segment tables are uploaded here, once per
    call."""
    ptrs, cnts, nseg, _, dt = _seg_tables(tensors, counts, dtype)
    check(_lib().mlsl_hip_clip_scale_list(ptrs, cnts, nseg, DTYPE[dt],
                                          _f64_scalar(total, "total"), max_norm))


def clip_scale_list_tables(dev_ptrs, dev_offs, nseg, count, total, max_norm, dtype="f32"):
    """`clip_scale_list` over tables in DEVICE memory; see
    `quantize_gather_tables`."""
    pp, _ = _as_ptr_dtype(dev_ptrs)
    op_, _ = _as_ptr_dtype(dev_offs)
    check(_lib().mlsl_hip_clip_scale_list_tables(pp, op_, nseg, count, DTYPE[dtype],
                                                 _f64_scalar(total, "total"), max_norm))


def _adamw_args(lr, betas, eps, weight_decay, step, grad_scale, total, max_norm, out, replica,
                dtype):
    """The refusals the device and the host form share, and the ten float32
    scalars in AdamWScalars' order: each computed in double, rounded once."""
    if int(step) < 1:
        raise ValueError(f"step={step!r}: the bias corrections need a step count of at "
                         "least 1")
    if replica is not None and out is None:
        raise ValueError("replica without out: the delta to the replica has nowhere to go")
    if (total is None) != (max_norm is None):
        raise ValueError("total and max_norm go together: the squared norm and its bound")
    if dtype not in _LIST_ELEM_BYTES:
        raise ValueError(f"gradient dtype {dtype!r}: adamw_step supports f32/bf16/f16 only")
    b1, b2 = float(betas[0]), float(betas[1])
    return (ctypes.c_float * 10)(
        grad_scale, 0.0 if max_norm is None else max_norm, b1, b2, 1.0 - b1, 1.0 - b2,
        lr / (1.0 - b1 ** step), math.sqrt(1.0 - b2 ** step), eps, 1.0 - lr * weight_decay)


def adamw_elems_per_trip():
    """Elements one launch of `adamw_step` covers before its grid-stride loop
    takes a second trip (the same for every gradient dtype)."""
    n = ctypes.c_size_t(0)
    check(_lib().mlsl_hip_adamw_elems_per_trip(ctypes.byref(n)))
    return n.value


def adamw_step(grad, p, m, v, count, *, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01,
               step, grad_scale=1.0, total=None, max_norm=None, out=None, replica=None,
               dtype=None, path=None):
    """One fused AdamW step over the first `count` elements of a flat shard,
    in one pass and in float32 operations that each round once (no fma):

        coef = min(1, max_norm / (sqrt(total) * grad_scale + 1e-6))  # 1 without total
        g'   = (float(grad) * grad_scale) * coef
        m    = m * b1 + g' * (1 - b1)
        v    = v * b2 + (g' * g') * (1 - b2)
        p    = p * (1 - lr * weight_decay)
               - (m / (sqrt(v) / sqrt(1 - b2**step) + eps)) * (lr / (1 - b1**step))

    `grad` is f32, bf16 or f16 and only read. `p`, `m`, `v` are float32,
    16-byte aligned and updated in place: the master weights and both moments.
    `total` is the unscaled squared norm as a device f64 scalar (`sumsq` leaves
    it so); the kernel reads it, the host does not. `out`, in grad's dtype,
    takes the rounded new p, or with `replica` (only read) the rounded
    p - replica. path=None moves grad, out and replica as vectors when all are
    16-byte aligned and element by element otherwise; "generic" and "fast" name
    the path, and "fast" on misaligned buffers is refused."""
    gp, d1 = _as_ptr_dtype(grad)
    dt = dtype or d1
    sc = _adamw_args(lr, betas, eps, weight_decay, step, grad_scale, total, max_norm, out,
                     replica, dt)
    state = []
    for name, t in (("p", p), ("m", m), ("v", v)):
        tp, td = _as_ptr_dtype(t)
        if td not in (None, "f32") or tp.value is None or tp.value % 16:
            raise ValueError(f"{name} must be a 16-byte aligned float32 buffer")
        state.append(tp)
    op_, _ = _as_ptr_dtype(out)
    rp, _ = _as_ptr_dtype(replica)
    check(_lib().mlsl_hip_adamw_step(gp, *state, op_, rp, count, DTYPE[dt],
                                     None if total is None else _f64_scalar(total, "total"),
                                     sc, _PATH4[path]))


def host_adamw_step(grad, p, m, v, count, *, lr, betas=(0.9, 0.999), eps=1e-8,
                    weight_decay=0.01, step, grad_scale=1.0, total=None, max_norm=None,
                    out=None, replica=None, dtype="f32"):
    """Host twin of `adamw_step` on numpy arrays: the same bits. bf16 and f16
    travel as uint16 bit patterns; p, m and v are float32 arrays; `total` is a
    Python float, the squared norm."""
    sc = _adamw_args(lr, betas, eps, weight_decay, step, grad_scale, total, max_norm, out,
                     replica, dtype)
    for name, a in (("p", p), ("m", m), ("v", v)):
        if str(getattr(a, "dtype", None)) != "float32":
            raise ValueError(f"{name} must be a float32 array")
    eb = _LIST_ELEM_BYTES[dtype]
    tot = None if total is None else ctypes.byref(ctypes.c_double(total))
    check(_lib().mlsl_host_adamw_step(
        _host_buf(grad, count * eb, "grad"), _host_buf(p, count * 4, "p"),
        _host_buf(m, count * 4, "m"), _host_buf(v, count * 4, "v"),
        None if out is None else _host_buf(out, count * eb, "out"),
        None if replica is None else _host_buf(replica, count * eb, "replica"),
        count, DTYPE[dtype], tot, sc))


_ELEM_BYTES = {"f32": 4, "bf16": 2}
_LIST_ELEM_BYTES = {"f32": 4, "bf16": 2, "f16": 2}   # the exact pair takes f16 too


def _host_seg_tables(arrays, counts, dtype, what, elem_bytes=_ELEM_BYTES):
    if dtype not in elem_bytes:
        if elem_bytes is _LIST_ELEM_BYTES:
            raise ValueError(f"dtype {dtype!r}: the exact list kernels support "
                             "f32/bf16/f16 only")
        raise ValueError(f"dtype {dtype!r}: the list codec supports f32/bf16 only")
    if len(arrays) != len(counts):
        raise ValueError(f"{len(arrays)} {what} but {len(counts)} counts")
    if not counts:
        raise ValueError("the tensor list is empty: at least one segment is needed")
    for j, n in enumerate(counts):
        if int(n) < 1:
            raise ValueError(f"counts[{j}] = {n}: every segment needs at least one element")
    eb = elem_bytes[dtype]
    ptrs = (ctypes.c_void_p * len(arrays))(
        *[_host_buf(a, int(n) * eb, f"{what}[{j}]").value
          for j, (a, n) in enumerate(zip(arrays, counts))])
    return (ptrs, (ctypes.c_size_t * len(counts))(*[int(n) for n in counts]), len(counts),
            sum(int(n) for n in counts))


def host_quantize_gather(arrays, counts, wire, err=None, block=256, dtype="f32"):
    """Host twin of `quantize_gather` on numpy arrays: the same bits."""
    _check_block(block)
    ptrs, cnts, nseg, total = _host_seg_tables(arrays, counts, dtype, "arrays")
    wp = _host_buf(wire, wire_bytes(total, block), "wire")
    ep = None if err is None else _host_buf(err, total * _ELEM_BYTES[dtype], "err")
    check(_lib().mlsl_host_quantize_gather(ptrs, cnts, nseg, ep, wp, block, DTYPE[dtype],
                                           1 if err is not None else 0))


def host_quantize_gather_shards(arrays, counts, wire, nshards, shard, err=None, block=256,
                                dtype="f32", wire_stride=None):
    """Host twin of `quantize_gather_shards` on numpy arrays: the same bits."""
    _check_block(block)
    ptrs, cnts, nseg, total = _host_seg_tables(arrays, counts, dtype, "arrays")
    nshards, shard, wire_stride = _shard_args(total, nshards, shard, wire_stride, block)
    wp = _host_buf(wire, (nshards - 1) * wire_stride + wire_bytes(shard, block), "wire")
    ep = None if err is None else _host_buf(err, nshards * shard * _ELEM_BYTES[dtype], "err")
    check(_lib().mlsl_host_quantize_gather_shards(ptrs, cnts, nseg, ep, wp, nshards, shard,
                                                  wire_stride, block, DTYPE[dtype],
                                                  1 if err is not None else 0))


def host_dequantize_scatter(wire, arrays, counts, block=256, dtype="f32", post_scale=1.0,
                            round_first=False):
    """Host twin of `dequantize_scatter` on numpy arrays: the same bits."""
    _check_block(block)
    ptrs, cnts, nseg, total = _host_seg_tables(arrays, counts, dtype, "arrays")
    wp = _host_buf(wire, wire_bytes(total, block), "wire")
    check(_lib().mlsl_host_dequantize_scatter(wp, ptrs, cnts, nseg, block, DTYPE[dtype],
                                              post_scale, 1 if round_first else 0))


def host_gather_list(arrays, counts, flat, dtype="f32"):
    """Host twin of `gather_list` on numpy arrays: the same bits."""
    ptrs, cnts, nseg, total = _host_seg_tables(arrays, counts, dtype, "arrays",
                                               _LIST_ELEM_BYTES)
    fp = _host_buf(flat, total * _LIST_ELEM_BYTES[dtype], "flat")
    check(_lib().mlsl_host_gather_list(ptrs, cnts, nseg, fp, DTYPE[dtype]))


def host_scatter_scale_list(flat, arrays, counts, dtype="f32", post_scale=1.0):
    """Host twin of `scatter_scale_list` on numpy arrays: the same bits, except
    that a bf16/f16 NaN that goes through the product (post_scale != 1) comes
    out as the quiet NaN of its sign."""
    ptrs, cnts, nseg, total = _host_seg_tables(arrays, counts, dtype, "arrays",
                                               _LIST_ELEM_BYTES)
    fp = _host_buf(flat, total * _LIST_ELEM_BYTES[dtype], "flat")
    check(_lib().mlsl_host_scatter_scale_list(fp, ptrs, cnts, nseg, DTYPE[dtype], post_scale))


def host_quantize_gather4(arrays, counts, wire, err=None, block=256, dtype="f32"):
    """Host twin of `quantize_gather4` on numpy arrays: the same bits."""
    _check_block4(block)
    ptrs, cnts, nseg, total = _host_seg_tables(arrays, counts, dtype, "arrays")
    wp = _host_buf(wire, wire_bytes(total, block, 4), "wire")
    ep = None if err is None else _host_buf(err, total * _ELEM_BYTES[dtype], "err")
    check(_lib().mlsl_host_quantize_gather4(ptrs, cnts, nseg, ep, wp, block, DTYPE[dtype],
                                            1 if err is not None else 0))


def host_quantize_gather_shards4(arrays, counts, wire, nshards, shard, err=None, block=256,
                                 dtype="f32", wire_stride=None):
    """Host twin of `quantize_gather_shards4` on numpy arrays: the same bits."""
    _check_block4(block)
    ptrs, cnts, nseg, total = _host_seg_tables(arrays, counts, dtype, "arrays")
    nshards, shard, wire_stride = _shard_args(total, nshards, shard, wire_stride, block, 4)
    wp = _host_buf(wire, (nshards - 1) * wire_stride + wire_bytes(shard, block, 4), "wire")
    ep = None if err is None else _host_buf(err, nshards * shard * _ELEM_BYTES[dtype], "err")
    check(_lib().mlsl_host_quantize_gather_shards4(ptrs, cnts, nseg, ep, wp, nshards, shard,
                                                   wire_stride, block, DTYPE[dtype],
                                                   1 if err is not None else 0))


def host_dequantize_scatter4(wire, arrays, counts, block=256, dtype="f32", post_scale=1.0,
                             round_first=False):
    """Host twin of `dequantize_scatter4` on numpy arrays: the same bits."""
    _check_block4(block)
    ptrs, cnts, nseg, total = _host_seg_tables(arrays, counts, dtype, "arrays")
    wp = _host_buf(wire, wire_bytes(total, block, 4), "wire")
    check(_lib().mlsl_host_dequantize_scatter4(wp, ptrs, cnts, nseg, block, DTYPE[dtype],
                                               post_scale, 1 if round_first else 0))


def _host_buf(arr, need_bytes, what):
    """Pointer of a C-contiguous numpy array holding at least need_bytes."""
    if not hasattr(arr, "__array_interface__"):
        raise TypeError(f"{what}: numpy array expected, got {type(arr)}")
    if not arr.flags["C_CONTIGUOUS"] or arr.nbytes < need_bytes:
        raise ValueError(f"{what}: need a contiguous array of >= {need_bytes} bytes")
    return ctypes.c_void_p(arr.__array_interface__["data"][0])


def _check_block(block):
    # the C entry points reject it too; here before wire_bytes() divides by it
    if block == 0 or block % 4:
        raise ValueError(f"quantization block of {block} elements is not supported "
                         "(must be a non-zero multiple of 4)")


def host_quantize(inp, wire, count, err=None, block=256, dtype="f32"):
    """Host codec (csrc/comm/quant.cpp) on numpy arrays; bf16 travels as
    uint16 bit patterns. Same wire format as `quantize`."""
    _check_block(block)
    eb = _ELEM_BYTES[dtype]
    ip = _host_buf(inp, count * eb, "inp")
    wp = _host_buf(wire, wire_bytes(count, block), "wire")
    ep = None if err is None else _host_buf(err, count * eb, "err")
    check(_lib().mlsl_host_quantize(ip, ep, wp, count, block, DTYPE[dtype],
                                    1 if err is not None else 0))


def host_dequantize(wire, out, count, block=256, dtype="f32"):
    _check_block(block)
    wp = _host_buf(wire, wire_bytes(count, block), "wire")
    op_ = _host_buf(out, count * _ELEM_BYTES[dtype], "out")
    check(_lib().mlsl_host_dequantize(wp, op_, count, block, DTYPE[dtype]))


def host_quant_accum(acc_wire, wire, count, block=256):
    _check_block(block)
    ap = _host_buf(acc_wire, wire_bytes(count, block), "acc_wire")
    wp = _host_buf(wire, wire_bytes(count, block), "wire")
    check(_lib().mlsl_host_quant_accum(ap, wp, count, block))


def host_quant_sum_dequant(a_wire, b_wire, out, count, block=256, dtype="f32"):
    """Host twin of `quant_sum_dequant` on numpy arrays."""
    _check_block(block)
    ap = _host_buf(a_wire, wire_bytes(count, block), "a_wire")
    bp = _host_buf(b_wire, wire_bytes(count, block), "b_wire")
    op_ = _host_buf(out, count * _ELEM_BYTES[dtype], "out")
    check(_lib().mlsl_host_quant_sum_dequant(ap, bp, op_, count, block, DTYPE[dtype]))


def host_quant_sum_dequant_n(wires, out, count, block=256, dtype="f32"):
    """Host twin of `quant_sum_dequant_n` on numpy arrays: the same bits."""
    _check_block(block)
    ptrs = (ctypes.c_void_p * len(wires))(
        *[_host_buf(w, wire_bytes(count, block), f"wires[{i}]").value
          for i, w in enumerate(wires)])
    op_ = _host_buf(out, count * _ELEM_BYTES[dtype], "out")
    check(_lib().mlsl_host_quant_sum_dequant_n(ptrs, len(wires), op_, count, block,
                                               DTYPE[dtype]))


def host_quant_sum_requant_n(wires, dst, nunits, block=256):
    """Host twin of `quant_sum_requant_n` on numpy arrays: the same bits."""
    _check_block(block)
    need = nunits * (block + 8)
    ptrs = (ctypes.c_void_p * len(wires))(
        *[_host_buf(w, need, f"wires[{i}]").value for i, w in enumerate(wires)])
    dp = _host_buf(dst, need, "dst")
    check(_lib().mlsl_host_quant_sum_requant_n(ptrs, len(wires), dp, nunits, block))


def host_quantize4(inp, wire, count, err=None, block=256, dtype="f32"):
    """Host twin of `quantize4` on numpy arrays: the same bits."""
    _check_block4(block)
    eb = _ELEM_BYTES[dtype]
    ip = _host_buf(inp, count * eb, "inp")
    wp = _host_buf(wire, wire_bytes(count, block, 4), "wire")
    ep = None if err is None else _host_buf(err, count * eb, "err")
    check(_lib().mlsl_host_quantize4(ip, ep, wp, count, block, DTYPE[dtype],
                                     1 if err is not None else 0))


def host_dequantize4(wire, out, count, block=256, dtype="f32"):
    """Host twin of `dequantize4` on numpy arrays: the same bits."""
    _check_block4(block)
    wp = _host_buf(wire, wire_bytes(count, block, 4), "wire")
    op_ = _host_buf(out, count * _ELEM_BYTES[dtype], "out")
    check(_lib().mlsl_host_dequantize4(wp, op_, count, block, DTYPE[dtype]))


def host_quant_sum_dequant_n4(wires, out, count, block=256, dtype="f32"):
    """Host twin of `quant_sum_dequant_n4` on numpy arrays: the same bits."""
    _check_block4(block)
    ptrs = (ctypes.c_void_p * len(wires))(
        *[_host_buf(w, wire_bytes(count, block, 4), f"wires[{i}]").value
          for i, w in enumerate(wires)])
    op_ = _host_buf(out, count * _ELEM_BYTES[dtype], "out")
    check(_lib().mlsl_host_quant_sum_dequant_n4(ptrs, len(wires), op_, count, block,
                                                DTYPE[dtype]))


def host_quant_sum_requant_n4(wires, dst, nunits, block=256):
    """Host twin of `quant_sum_requant_n4` on numpy arrays: the same bits."""
    _check_block4(block)
    need = nunits * (block // 2 + 8)
    ptrs = (ctypes.c_void_p * len(wires))(
        *[_host_buf(w, need, f"wires[{i}]").value for i, w in enumerate(wires)])
    dp = _host_buf(dst, need, "dst")
    check(_lib().mlsl_host_quant_sum_requant_n4(ptrs, len(wires), dp, nunits, block))


def host_dequantize_segments(wire, out, count, nseg, block=256, dtype="f32",
                             accumulate=False):
    """Host twin of `dequantize_segments` on numpy arrays: the same bits."""
    _check_block(block)
    wp = _host_buf(wire, nseg * wire_bytes(count, block), "wire")
    op_ = _host_buf(out, nseg * count * _ELEM_BYTES[dtype], "out")
    check(_lib().mlsl_host_dequantize_segments(wp, nseg, op_, count, block, DTYPE[dtype],
                                               1 if accumulate else 0))


def host_dequantize_segments4(wire, out, count, nseg, block=256, dtype="f32",
                              accumulate=False):
    """Host twin of `dequantize_segments4` on numpy arrays: the same bits."""
    _check_block4(block)
    wp = _host_buf(wire, nseg * wire_bytes(count, block, 4), "wire")
    op_ = _host_buf(out, nseg * count * _ELEM_BYTES.get(dtype, 8), "out")
    check(_lib().mlsl_host_dequantize_segments4(wp, nseg, op_, count, block, DTYPE[dtype],
                                                1 if accumulate else 0))


def pack(src, dst, *, mb_offset, mb_count, fm_offset, fm_count, fm_size,
         buf_offset, local_fm_count, local_mb_count, dtype):
    sp, _ = _as_ptr_dtype(src)
    dp, _ = _as_ptr_dtype(dst)
    check(_lib().mlsl_hip_pack(sp, dp, mb_offset, mb_count, fm_offset, fm_count,
                               fm_size, buf_offset, local_fm_count, local_mb_count,
                               DTYPE[dtype]))


def unpack(src, dst, *, mb_offset, mb_count, fm_offset, fm_count, fm_size,
           buf_offset, local_fm_count, local_mb_count, dtype):
    sp, _ = _as_ptr_dtype(src)
    dp, _ = _as_ptr_dtype(dst)
    check(_lib().mlsl_hip_unpack(sp, dp, mb_offset, mb_count, fm_offset, fm_count,
                                 fm_size, buf_offset, local_fm_count, local_mb_count,
                                 DTYPE[dtype]))
