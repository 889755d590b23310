"""Standalone CDNA4 kernel ops (device-pointer API over the HIP kernels in
csrc/hip/kernels.hip): local reductions, int8 block quantization with error
feedback, and pack/unpack. Used by GPU numerics tests and by consumers that
want the fused kernels without the full Session machinery.

Buffers: torch CUDA tensors, raw integer device pointers, or anything with
``data_ptr()``. The ``host_*`` functions run the host codec of
csrc/comm/quant.cpp (same wire format) on numpy arrays.
"""
import ctypes

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
        L.mlsl_hip_dequantize_segments.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p,
                                                   c.c_size_t, c.c_size_t, c.c_int, c.c_int]
        L.mlsl_host_dequantize_segments.argtypes = L.mlsl_hip_dequantize_segments.argtypes
        L.mlsl_hip_dequantize_segments.restype = c.c_int
        L.mlsl_host_dequantize_segments.restype = c.c_int
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
        for n in ("mlsl_hip_quantize_gather_shards", "mlsl_host_quantize_gather_shards",
                  "mlsl_hip_quantize_gather_shards_tables"):
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


def wire_bytes(count, block=256):
    """Bytes of the int8 wire format for `count` elements."""
    nblocks = (count + block - 1) // block
    return nblocks * (block + 8)


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


def _shard_args(total, nshards, shard, wire_stride, block):
    """(nshards, shard, wire_stride) checked; wire_stride=None is one shard's
    wire bytes rounded up to 16."""
    nshards, shard = int(nshards), int(shard)
    if nshards < 1 or shard * nshards < total:
        raise ValueError(f"shard * nshards < total: {nshards} shards of {shard} elements "
                         f"do not hold {total}")
    need = wire_bytes(shard, block)
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


_ELEM_BYTES = {"f32": 4, "bf16": 2}


def _host_seg_tables(arrays, counts, dtype, what):
    if dtype not in _ELEM_BYTES:
        raise ValueError(f"dtype {dtype!r}: the list codec supports f32/bf16 only")
    if len(arrays) != len(counts):
        raise ValueError(f"{len(arrays)} {what} but {len(counts)} counts")
    if not counts:
        raise ValueError("the tensor list is empty: at least one segment is needed")
    for j, n in enumerate(counts):
        if int(n) < 1:
            raise ValueError(f"counts[{j}] = {n}: every segment needs at least one element")
    eb = _ELEM_BYTES[dtype]
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


def host_dequantize_segments(wire, out, count, nseg, block=256, dtype="f32",
                             accumulate=False):
    """Host twin of `dequantize_segments` on numpy arrays: the same bits."""
    _check_block(block)
    wp = _host_buf(wire, nseg * wire_bytes(count, block), "wire")
    op_ = _host_buf(out, nseg * count * _ELEM_BYTES[dtype], "out")
    check(_lib().mlsl_host_dequantize_segments(wp, nseg, op_, count, block, DTYPE[dtype],
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
