// Host-callable launchers for the CDNA4 HIP kernels (gfx950).
#pragma once

#include <hip/hip_runtime.h>

#include "../core/types.hpp"

namespace mlsl {

// dst[i] op= src[i] for count elements, on `stream`.
// Memory-bound: vectorized 16-byte accesses, grid-stride, XCD-friendly
// grid sizing (see kernels.hip).
void LaunchReduce(void* dst, const void* src, size_t count, DataType dt,
                  ReduceOp op, hipStream_t stream);

// f32 SUM with nontemporal loads/stores (A/B benchmarking).
void LaunchReduceNT(void* dst, const void* src, size_t count, hipStream_t stream);
void LaunchReduceNT2(void* dst, const void* src, size_t count, hipStream_t stream);

// dst = a + b elementwise into a third buffer (out-of-place variant used by
// fused pipelines).
void LaunchReduceOut(void* dst, const void* a, const void* b, size_t count,
                     DataType dt, ReduceOp op, hipStream_t stream);

// Streaming device-to-device copy. For large 16-byte-aligned transfers a
// nontemporal grid-stride kernel beats hipMemcpyAsync's blit path on HBM3E
// (same reason the NT reduce wins: no L2 retention for stream-once data);
// misaligned or small copies fall back to hipMemcpyAsync on `stream`.
void LaunchCopy(void* dst, const void* src, size_t bytes, hipStream_t stream);
void LaunchCopyVariant(void* dst, const void* src, size_t bytes, bool nt,
                       hipStream_t stream);

// --- int8 block quantization with error feedback (quant/quant.c contract,
//     fused into the allreduce path; see comm/quant.cpp) ---
// Wire block layout: [float scale][float reserved][int8 x block_elems].
// in: fp32/bf16 gradients; err: same shape residual carried across steps
// (error feedback); out: packed wire blocks.
void LaunchQuantize(const void* in, void* err, void* wire, size_t count,
                    size_t block_elems, DataType dt, bool use_err,
                    hipStream_t stream);
// Dequantize wire blocks into out (fp32/bf16).
void LaunchDequantize(const void* wire, void* out, size_t count,
                      size_t block_elems, DataType dt, hipStream_t stream);
void LaunchQuantizeF32NT(const void* in, void* err, void* wire, size_t count,
                         size_t block_elems, hipStream_t stream);
void LaunchDequantizeNT(const void* wire, void* out, size_t count,
                        size_t block_elems, DataType dt, hipStream_t stream);
// Compressed-domain accumulate: acc_wire += wire (dequant-sum-requant per
// block, matching the reference's reduce_sum plugin hook quant/quant.c:89-94).
void LaunchQuantAccum(void* acc_wire, const void* wire, size_t count,
                      size_t block_elems, hipStream_t stream);
// Fused last hop of the quantized reduce-scatter:
// out[i] = dequant(a_wire)[i] + dequant(b_wire)[i] for i < count, in the
// element type (fp32/bf16). Neither wire is written; the sum is not
// requantized. Outputs of 128 MiB and more are stored nontemporally on the
// fast path; the NT variant does so at any size (A/B hook).
void LaunchQuantSumDequant(const void* a_wire, const void* b_wire, void* out,
                           size_t count, size_t block_elems, DataType dt,
                           hipStream_t stream);
void LaunchQuantSumDequantNT(const void* a_wire, const void* b_wire, void* out,
                             size_t count, size_t block_elems, DataType dt,
                             hipStream_t stream);
// N-way fan-in of the one-shot quantized reduce-scatter: out[i] = the sum of
// dequant(wires[r])[i] over r = 0..nwires-1 (1 to 8 wires, fp32/bf16 out).
// Per element acc = +0, then acc = fma(q_r, scale_r, acc) in wire order,
// rounded once into the element type; the host twin computes the same bits.
// `wires` is a host array read during the call; no wire is written and
// nothing past out[count) is.
void LaunchQuantSumDequantN(const void* const* wires, int nwires, void* out, size_t count,
                            size_t block_elems, DataType dt, hipStream_t stream);
// The owner's step of the two-shot quantized allreduce: dst_wire = the sum of
// dequant(wires[r]) over r = 0..nwires-1 (1 to 8 wires), requantized once,
// over `nunits` whole wire units of block_elems + 8 bytes. No element count
// and no dtype: the padding of a partial block is zero in every wire, sums to
// zero and requantizes to zero. Per element acc = +0, then
// acc = fma(q_r, scale_r, acc) in wire order; the block's scale is
// max|acc| / 127 (1 for an all-zero block), q = clamp(rint(acc * (1 / scale)));
// the header's second word is 0. The host twin computes the same bits.
// Wires must be 4-byte aligned; 8-byte aligned wires of 256-blocks take a
// register-resident fast path. dst_wire may be EXACTLY one of the wires (the
// sum then replaces it in place) or overlap none; never partially. Stores
// are plain: the destination is handed to peers next. `wires` is a host array
// read during the call.
void LaunchQuantSumRequantN(const void* const* wires, int nwires, void* dst_wire,
                            size_t nunits, size_t block_elems, hipStream_t stream);
// Finish of the quantized all-gather, one launch for any nseg >= 1: `wire`
// holds nseg segment wires of NumBlocks(count) blocks each, one after the
// other and every one on a block grid of its own (a partial last block is
// followed by the next segment's block 0); segment j goes to
// out[j * count, (j + 1) * count). Assigned with the bits of LaunchDequantize,
// or with `accumulate` as out = fma(q, scale, out) in float, rounded once
// into the element type (fp32/bf16). Vector stores are decided per segment,
// so `out` and count may have any alignment. The wire is not written and
// nothing past out[nseg * count) is. Outputs of 128 MiB and more are stored
// nontemporally on the fast path (LaunchQuantSumDequant's rule).
// Whole 256-blocks in assign mode are contiguous whole blocks, which
// LaunchDequantize's flat kernels decode to the same bits; this launcher
// keeps its own kernel there: at 64 Mi elements it took 0.78 of the flat f32
// kernel's time and the same time as the bf16 one (docs/BENCHMARKS.md).
void LaunchDequantizeSegments(const void* wire, size_t nseg, void* out, size_t count,
                              size_t block_elems, DataType dt, bool accumulate,
                              hipStream_t stream);

// Prologue and finish of the quantized allreduce over a list of tensors. The
// concatenation V of the nseg tensors (count elements in all, fp32/bf16) is
// never materialised: tensor j holds V[seg_offs[j], seg_offs[j + 1]). Both
// tables are DEVICE memory: nseg + 1 prefix offsets in elements (seg_offs[0]
// == 0, seg_offs[nseg] == count, every tensor at least one element) and nseg
// tensor pointers, each aligned to the element size only. Boundaries may fall
// anywhere inside a wire block.
// Gather: `wire`, and `err` (one flat residual of count elements in V's
// order) when use_err, get the bytes LaunchQuantize writes for V; the tensors
// are only read.
void LaunchQuantizeGather(const void* const* seg_ptrs, const uint64_t* seg_offs, size_t nseg,
                          void* err, void* wire, size_t count, size_t block_elems,
                          DataType dt, bool use_err, hipStream_t stream);
// Prologue of the quantized reduce-scatter over a list of tensors. V' is V (the
// tables above, `total` elements) followed by zeros up to nshards * shard
// elements (shard * nshards >= total). One launch writes, for every shard j,
// the bytes LaunchQuantize writes for V'[j * shard, (j + 1) * shard) to wire +
// j * wire_stride (wire_stride: a multiple of 4, at least one shard's wire
// bytes; the bytes between two shards' wires are not written) and, when
// use_err, to err + j * shard: the residual is flat in V' order, nshards * shard
// elements. A shard may begin or end inside a tensor. An element at or past
// `total` quantizes as 0, is read through no pointer, and its residual, +0
// from the start, is neither read nor written.
void LaunchQuantizeGatherShards(const void* const* seg_ptrs, const uint64_t* seg_offs,
                                size_t nseg, void* err, void* wire, size_t total,
                                size_t nshards, size_t shard, size_t wire_stride,
                                size_t block_elems, DataType dt, bool use_err,
                                hipStream_t stream);
// Scatter: every element becomes Encode((q * scale) * post_scale), both
// products rounded to float and one final rounding for bf16: with post_scale
// == 1.0f the bits of LaunchDequantize. The wire is only read and no byte
// outside the tensors is written.
// round_first (bf16; nothing changes for fp32): q * scale is rounded to bf16
// before the scaling, Encode(Decode(Encode(q * scale)) * post_scale): the bits
// of LaunchDequantize followed by a float multiplication of the stored
// elements. The request uses it, so that a list request and a flat request
// plus a scaling of its result agree bit for bit whatever post_scale is.
void LaunchDequantizeScatter(const void* wire, void* const* seg_ptrs,
                             const uint64_t* seg_offs, size_t nseg, size_t count,
                             size_t block_elems, DataType dt, float post_scale,
                             bool round_first, hipStream_t stream);

// Strided pack/unpack between layer layout [mb][fm][fmSize] and a contiguous
// comm buffer block (CommBlockInfo contract; reference computes the shapes,
// the consumer does the copy — tests/examples/mlsl_test/mlsl_test.cpp:214-254.
// Here it is a library kernel so GPU consumers get a fused path).
struct PackBlockDesc {
    size_t mb_offset, mb_count;
    size_t fm_offset, fm_count;
    size_t fm_size;          // elements per feature map
    size_t buf_offset;       // element offset in the comm buffer
    size_t local_fm_count;   // feature maps per sample in the local layout
    size_t local_mb_count;   // samples in the local layout
};
void LaunchPack(const void* src, void* dst, const PackBlockDesc& d, DataType dt,
                hipStream_t stream);
void LaunchUnpack(const void* src, void* dst, const PackBlockDesc& d, DataType dt,
                  hipStream_t stream);

// --- fused transport kernels (IPC p2p path) ---
// Optional flag-wait prologue: every workgroup polls *mbox >= target
// before touching the payload (abort word + wall-clock escape as in
// LaunchWaitFlag). Fusing the wait into the payload kernel removes two
// kernel launches per transport sub-message.
struct XferPoll {
    const void* mbox;
    uint64_t target;
    const void* abort_word;
    void* status;
    uint64_t max_ticks;
};
// Streaming byte copy with optional poll prologue (16-B lanes; NT loads of
// the local source, plain stores into the hand-off slot).
void LaunchXferCopy(void* dst, const void* src, size_t bytes,
                    const XferPoll* poll, hipStream_t stream);
// dst op= slot (other==null) or dst = slot op other, with optional poll.
// Returns false when dtype isn't covered (caller uses LaunchWaitFlag +
// LaunchReduce instead).
bool LaunchXferReduce(void* dst, const void* slot, const void* other, size_t n,
                      DataType dt, ReduceOp op, const XferPoll* poll,
                      hipStream_t stream);

// Fully-fused small-message transport kernels: poll + payload + grid-
// completion counter + flag publish, in ONE launch with a bounded grid
// (spinners can never starve the peer's kernels). ctr_target is the
// ABSOLUTE cumulative workgroup-add count for that counter (the host
// accumulates kXferFusedGrid / FanOutWgsPerPeer() per emitted kernel, so
// kernels with different grids can share an edge counter).
// Recv `mode`: COPY (n = BYTES), REDUCE into dst, REDUCE_OUT = slot op
// other (n = elements); returns false for uncovered dtypes.
enum class FusedConsume : int { COPY = 0, REDUCE = 1, REDUCE_OUT = 2 };
constexpr uint32_t kXferFusedGrid = 32;   // wgs per fused send/recv kernel
// wgs per peer in the fan-out: full grid for one peer, split for many
int FanOutWgsPerPeer(int npeers);
void LaunchXferSendFused(void* slot, const void* src, size_t bytes,
                         const XferPoll* bp, void* ctr, uint64_t ctr_target,
                         void* in_mbox, uint64_t seq, hipStream_t stream);
bool LaunchXferRecvFused(void* dst, const void* slot, const void* other,
                         size_t n, DataType dt, ReduceOp op, FusedConsume mode,
                         const XferPoll* wp, void* ctr, uint64_t ctr_target,
                         void* ack_mbox, uint64_t seq, hipStream_t stream);

// Fused arrival-wait + compressed-domain block accumulate for the
// quantized ring's consume step (count in ELEMENTS of the quant blocks).
void LaunchXferRecvQuantAccum(void* acc, const void* slot, size_t count,
                              size_t block_elems, const XferPoll* wp,
                              void* ctr, uint64_t ctr_target, void* ack_mbox,
                              uint64_t seq, hipStream_t stream);

// One-shot (direct) allreduce fan kernels: up to 8 peers per launch.
// Fan-out pushes the payload into every peer slot (per-peer backpressure
// + publish); fan-in waits all arrivals, reduces them into dst in one
// pass, and publishes every ack (uses the dedicated `ctr`).
struct FanPeer {
    void* slot;
    void* flag;            // publish target (in_flag for send, ack for recv)
    uint64_t flag_val;
    const void* wait_mbox; // backpressure (send, nullable) / arrival (recv)
    uint64_t wait_target;
    void* ctr;             // per-peer counter (fan-out only)
    uint64_t ctr_target;   // absolute adds target
};
void LaunchFanOutSend(const void* src, size_t bytes, const FanPeer* peers,
                      int npeers, const XferPoll* abort_info,
                      hipStream_t stream);
bool LaunchFanInReduce(void* dst, size_t n, DataType dt, ReduceOp op,
                       const FanPeer* peers, int npeers, void* ctr,
                       uint64_t ctr_target, const XferPoll* abort_info,
                       hipStream_t stream);

// --- IPC p2p transport flag primitives ---
// Stream-blocking wait until *mbox >= target (system-scope acquire), with a
// host abort word and a wall-clock bound (ticks of the 100 MHz constant
// clock); on abort/timeout writes 1 to `status` (pinned) and returns.
void LaunchWaitFlag(const void* mbox, uint64_t target, const void* abort_word,
                    void* status, uint64_t max_ticks, hipStream_t stream);
// System-scope release store of a new sequence value.
void LaunchSetFlag(void* mbox, uint64_t val, hipStream_t stream);

}  // namespace mlsl
