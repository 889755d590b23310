// Plan of one compressed (int8-quantized) chunk: where its wire, schedule
// scratch and error-feedback residual live, how the send buffer is cut into
// quantized segments, and which kernel finishes which wires. Built once per
// chunk at Setup; the host executor (request.cpp) and every device executor
// (device_comm.cpp) read it and derive none of this themselves.
//
// Layout from the chunk base, each region padded to 16 bytes so that the
// vectorized quant kernels' fast paths apply (wire blocks are block + 8
// bytes, so raw offsets are only 8-byte aligned):
//   [0, nseg * seg_wire)        wire: the quantized image of the whole send
//                               buffer; the schedule's SEND and RECV refs
//                               address it
//   [scratch_off, + tmp_bytes)  the schedule's TMP space
//   [err_off, + nseg * seg_bytes)  residual, one element per send element;
//                               absent (0 bytes) where `residual` is false
//
// The prologue quantizes send segment j (seg_bytes apart in the send buffer
// and the residual) into wire segment send_seg + j (seg_wire apart), each on
// a block grid of its own and with the residual only where `residual` says
// so, before anything writes the recv buffer: the two may alias anywhere.
// Then the schedule runs. Its local ops are REDUCE (QuantAccum of the step's
// own two ranges) and, in the two-shot allreduce only, one SUMQ: the
// sumq_nwires wires at sumq_wire_off[], sumq_units units each, are summed in
// that order and requantized once into sumq_dst_off, which is one of them
// (the own range, at position `me`; the others are the arrival slots in TMP).
// A rank that owns no units has sumq_units == 0 and skips the op.
// Then the finish writes `count` elements, or out_segs * count for SCATTER:
//   DEQUANT  allreduce (ring or two-shot: the whole wire at wire_off[0] = 0),
//            and any op on a group of one: dequantize wire_off[0]
//   SUM2     ring reduce-scatter: the partial sum that arrived last
//            (wire_off[0], in TMP) plus this rank's own segment (wire_off[1]),
//            one fused kernel
//   SUMN     one-shot reduce-scatter (fan_in > 0): the fan_in arrived wires
//            and the own segment in ascending group rank, own at position
//            `me`, summed once by the N-way kernel
//   SCATTER  all-gather: one send segment in, quantized into wire segment
//            `me`; the whole wire (wire_off[0] = 0) is out_segs segments,
//            rank j's at j * seg_wire, and the segmented dequantize writes
//            segment j to recv + j * seg_bytes, or adds it there with one fma
//            per element when `accumulate`. The own segment takes the same
//            path from its own wire, so recv comes out bit-identical on all
//            ranks. No residual: an error carried from one start to the next
//            suits gradient sums; on gathered values it would add one
//            start's rounding error to the next start's unrelated data.
// Host only: no HIP, no Context.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../core/types.hpp"
#include "schedule.hpp"

namespace mlsl {

enum class QuantFinish : uint8_t { DEQUANT, SUM2, SUMN, SCATTER };
// How (and whether) a chunk is an all-gather: MakeQuantPlan's last argument.
enum class QuantGather : uint8_t { NONE, ASSIGN, ACCUMULATE };

struct QuantPlan {
    size_t block = 0, count = 0;       // wire block elems; elements per segment (= result elems)
    size_t nseg = 1;                   // send segments (N for reduce-scatter, else 1)
    size_t send_seg = 0;               // wire segment of send segment 0 (`me` for all-gather)
    bool residual = true;              // the prologue carries an error-feedback residual
    size_t out_segs = 1;               // SCATTER: output segments, seg_bytes apart in recv
    bool accumulate = false;           // SCATTER: recv += dequantized, not recv =
    size_t seg_bytes = 0, seg_wire = 0;   // strides in send buffer/residual, and in the wire
    size_t scratch_off = 0, err_off = 0, bytes = 0;   // the wire region is at 0
    QuantFinish finish = QuantFinish::DEQUANT;
    int nwires = 1;                    // 1, 2, or fan_in + 1
    size_t wire_off[kQuantRsDirectMaxRanks] = {};   // in the order the finish sums them
    // The schedule's SUMQ step (two-shot allreduce); sumq_nwires == 0 where the
    // schedule has none. Offsets from the chunk base, wires in summing order
    // (ascending group rank, the own range at position `me`).
    int sumq_nwires = 0;
    size_t sumq_wire_off[kQuantRsDirectMaxRanks] = {};
    size_t sumq_dst_off = 0;           // the own range: one of sumq_wire_off
    size_t sumq_units = 0;             // wire units per wire; 0: this rank owns nothing
};

// `sch` is a *Units schedule of rank `me`; `count` elements of `elem_size`
// bytes per segment; `nseg` is the number of wire segments (the send segments
// of a reduce-scatter, the output segments of an all-gather, which `gather`
// marks). Throws where the schedule does not fit a finish.
QuantPlan MakeQuantPlan(const Schedule& sch, size_t nseg, size_t me, size_t count,
                        size_t elem_size, QuantGather gather = QuantGather::NONE);

// The plan's wire tables as pointers from the chunk base `base`, for the
// N-way kernels and their host twins: the finish's nwires, the SUMQ step's
// sumq_nwires. Entries past those counts are left alone.
inline void FinishWires(const QuantPlan& p, const uint8_t* base,
                        const void* (&wires)[kQuantRsDirectMaxRanks]) {
    for (int k = 0; k < p.nwires; ++k) wires[k] = base + p.wire_off[k];
}
inline void SumqWires(const QuantPlan& p, const uint8_t* base,
                      const void* (&wires)[kQuantRsDirectMaxRanks]) {
    for (int k = 0; k < p.sumq_nwires; ++k) wires[k] = base + p.sumq_wire_off[k];
}

}  // namespace mlsl
