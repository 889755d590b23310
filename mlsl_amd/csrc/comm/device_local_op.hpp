// What the two device schedule walkers (the RCCL one in device_comm.cpp and
// the IPC-window one in p2p_transport.cpp) do alike: resolve a schedule range
// to a device pointer, and launch a step's unfused local op.
#pragma once

#include <hip/hip_runtime.h>

#include "../hip/kernels.hpp"
#include "quant_plan.hpp"
#include "schedule.hpp"

namespace mlsl {

inline uint8_t* SpacePtr(const BufRef& b, const uint8_t* sbase, uint8_t* rbase, uint8_t* tmp) {
    switch (b.space) {
        case Space::SEND: return const_cast<uint8_t*>(sbase) + b.off;
        case Space::RECV: return rbase + b.off;
        case Space::TMP: return tmp + b.off;
    }
    return nullptr;
}

// The local op of `st` over its resolved ranges: COPY, the plan's SUMQ, the
// compressed-domain accumulate of a compressed chunk (`plan.block` > 0, units
// of `wire_unit` bytes), or the reduce. `plan_base` is where the plan's
// regions start: a compressed chunk's SEND base. `nt` picks the nontemporal
// copy kernel.
inline void LaunchLocalOp(const Step& st, uint8_t* dst, uint8_t* src, const QuantPlan& plan,
                          uint8_t* plan_base, DataType dtype, ReduceOp rop, size_t wire_unit,
                          hipStream_t s, bool nt) {
    if (st.local == Step::LocalOp::COPY) {
        if (dst == src) return;
        if (nt) LaunchCopy(dst, src, st.local_src.bytes, s);
        else LaunchCopyVariant(dst, src, st.local_src.bytes, false, s);
    } else if (st.local == Step::LocalOp::SUMQ) {
        const void* wires[kQuantRsDirectMaxRanks];
        SumqWires(plan, plan_base, wires);
        LaunchQuantSumRequantN(wires, plan.sumq_nwires, plan_base + plan.sumq_dst_off,
                               plan.sumq_units, plan.block, s);
    } else if (plan.block > 0) {
        LaunchQuantAccum(dst, src, (st.local_dst.bytes / wire_unit) * plan.block, plan.block, s);
    } else {
        LaunchReduce(dst, src, st.local_dst.bytes / DtypeSize(dtype), dtype, rop, s);
    }
}

}  // namespace mlsl
