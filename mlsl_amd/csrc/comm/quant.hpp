// int8 block quantization with error feedback — host reference
// implementation, semantics-identical to the CDNA4 kernels
// (csrc/hip/kernels.hip). Contract parity with the reference's compression
// plugin interface (quant/quant.c:57-94: quantize/dequantize/reduce_sum over
// fixed-size blocks, error-feedback diff buffer per gradient buffer).
//
// Wire block layout: [f32 scale][f32 reserved][int8 x block_elems].
#pragma once

#include <cstddef>
#include <cstdint>

#include "../core/types.hpp"

namespace mlsl {

inline size_t QuantWireBytes(size_t count, size_t block) {
    return ((count + block - 1) / block) * (block + 8);
}

// in (+ err if non-null) -> wire; err updated to the residual.
void HostQuantize(const void* in, void* err, void* wire, size_t count,
                  size_t block, DataType dt, bool use_err);
void HostDequantize(const void* wire, void* out, size_t count, size_t block,
                    DataType dt);
// acc_wire += wire in the compressed domain (dequant-sum-requant per block).
void HostQuantAccum(void* acc_wire, const void* wire, size_t count, size_t block);
// out = dequant(a_wire) + dequant(b_wire) in the element type, wires
// untouched: the quantized reduce-scatter's last hop (no requantization).
void HostQuantSumDequant(const void* a_wire, const void* b_wire, void* out,
                         size_t count, size_t block, DataType dt);
// out = sum over r of dequant(wires[r]), 1 to 8 wires, none written: the
// fan-in of the one-shot quantized reduce-scatter. Per element acc = +0, then
// acc = fmaf(q_r, scale_r, acc) in wire order, bit for bit what
// LaunchQuantSumDequantN computes.
void HostQuantSumDequantN(const void* const* wires, int nwires, void* out, size_t count,
                          size_t block, DataType dt);
// dst_wire = requantize(sum over r of dequant(wires[r])), 1 to 8 wires, over
// nunits whole wire units: the owner's step of the two-shot quantized
// allreduce. The sum is HostQuantSumDequantN's in float; the requantize is
// HostQuantize's (scale = max / 127 or 1, rint(v * (1 / scale)) clamped,
// second header word 0). dst_wire may be exactly one of the wires, or overlap
// none. Bit for bit what LaunchQuantSumRequantN computes.
void HostQuantSumRequantN(const void* const* wires, int nwires, void* dst_wire,
                          size_t nunits, size_t block);
// The finish of the quantized all-gather: `wire` holds nseg segment wires of
// QuantWireBytes(count, block) bytes each, every one on a block grid of its
// own, and segment j goes to out[j * count, (j + 1) * count): assigned as
// HostDequantize does it, or with `accumulate` as out = fmaf(q, scale, out)
// in float, rounded once into the element type. Any nseg >= 1; the wire is
// not written. Bit for bit what LaunchDequantizeSegments computes.
void HostDequantizeSegments(const void* wire, size_t nseg, void* out, size_t count,
                            size_t block, DataType dt, bool accumulate);

// Prologue and finish of the quantized allreduce over a list of tensors, whose
// concatenation V (count elements) is never materialised: tensor j holds
// V[seg_offs[j], seg_offs[j + 1]), with nseg + 1 prefix offsets in elements
// (seg_offs[0] == 0, seg_offs[nseg] == count, no empty tensor) and nseg
// pointers aligned to the element size only.
// Gather: wire, and the flat residual err of count elements when use_err, get
// the bytes HostQuantize writes for V; the tensors are only read. Bit for bit
// what LaunchQuantizeGather computes.
void HostQuantizeGather(const void* const* seg_ptrs, const uint64_t* seg_offs, size_t nseg,
                        void* err, void* wire, size_t count, size_t block, DataType dt,
                        bool use_err);
// Prologue of the quantized reduce-scatter over a list of tensors: V' is V
// (`total` elements, the tables above) followed by zeros up to nshards * shard
// elements, and shard j of V' gets HostQuantize's bytes at wire + j *
// wire_stride and, when use_err, at err + j * shard (the residual is flat in
// V' order). wire_stride is a multiple of 4 and at least one shard's wire
// bytes; the bytes between two wires are not written. An element at or past
// `total` quantizes as 0, is read through no pointer, and its residual is
// neither read nor written. Bit for bit what LaunchQuantizeGatherShards
// computes.
void HostQuantizeGatherShards(const void* const* seg_ptrs, const uint64_t* seg_offs,
                              size_t nseg, void* err, void* wire, size_t total,
                              size_t nshards, size_t shard, size_t wire_stride, size_t block,
                              DataType dt, bool use_err);
// Scatter: every element becomes (q * scale) * post_scale, both products
// rounded to float and one final rounding for bf16; with post_scale == 1.0f
// the bits of HostDequantize. Only the tensors are written. Bit for bit what
// LaunchDequantizeScatter computes. round_first (bf16; nothing changes for
// f32): q * scale is rounded to bf16 before it is scaled, the bits of
// HostDequantize followed by a float multiplication of the stored elements;
// the request's finish uses it.
void HostDequantizeScatter(const void* wire, void* const* seg_ptrs, const uint64_t* seg_offs,
                           size_t nseg, size_t count, size_t block, DataType dt,
                           float post_scale, bool round_first = false);

// dlopen'd compression plugin (reference quant/quant.c ABI — Intel
// DL-comp style). Loaded once per lib_path; used by the HOST compressed
// path when QuantParams.lib_path is set. Signatures quant/quant.c:57-65.
struct QuantPluginApi {
    int (*quant)(void* src, void* dst, size_t count, void* diff,
                 int src_data_type, size_t comp_ratio, int method);
    int (*dequant)(void* src, void* dst, size_t count);
    int (*reduce_sum)(const void* in, void* inout, size_t block_count);
};
// nullptr when qp.lib_path is empty; throws if the library or a symbol
// cannot be loaded (reference ASSERTs the same way, quant.c:112-126).
const QuantPluginApi* LoadQuantPlugin(const QuantParams& qp);

}  // namespace mlsl
