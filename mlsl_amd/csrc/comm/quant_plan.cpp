#include "quant_plan.hpp"

namespace mlsl {

QuantPlan MakeQuantPlan(const Schedule& sch, size_t nseg, size_t me, size_t count,
                        size_t elem_size, QuantGather gather) {
    auto al16 = [](size_t x) { return (x + 15) & ~size_t(15); };
    const BufRef& res = sch.result;
    MLSL_CHECK(sch.quant_block > 0 && nseg > 0 && (nseg == 1 || me < nseg),
               "not a compressed chunk's schedule");
    QuantPlan p;
    p.block = sch.quant_block;
    p.count = count;
    p.seg_bytes = count * elem_size;
    p.seg_wire = sch.wire_bytes / nseg;
    p.scratch_off = al16(nseg * p.seg_wire);
    p.err_off = p.scratch_off + al16(sch.tmp_bytes);
    if (gather != QuantGather::NONE) {
        // one send segment in, quantized into this rank's place in the wire
        // with no residual; nseg segments out
        MLSL_CHECK(res.space != Space::TMP && res.off == 0 &&
                       res.bytes == sch.wire_bytes && sch.fan_in == 0 &&
                       sch.tmp_bytes == 0,
                   "a compressed all-gather's result is the whole wire");
        p.nseg = 1;
        p.send_seg = me;
        p.residual = false;
        p.out_segs = nseg;
        p.finish = QuantFinish::SCATTER;
        p.accumulate = gather == QuantGather::ACCUMULATE;
        p.wire_off[0] = 0;
        p.bytes = p.err_off;
        return p;
    }
    MLSL_CHECK((res.space == Space::TMP) == (nseg > 1),
               "a compressed result is in TMP exactly for a reduce-scatter on "
               "more than one rank");
    p.nseg = nseg;
    p.bytes = p.err_off + al16(nseg * p.seg_bytes);
    if (sch.fan_in > 0) {
        MLSL_CHECK(sch.fan_in + 1 == nseg && nseg <= kQuantRsDirectMaxRanks,
                   "one-shot fan-in takes one wire per rank, 8 at the most");
        p.finish = QuantFinish::SUMN;
        p.nwires = static_cast<int>(nseg);
        for (size_t r = 0; r < nseg; ++r)
            p.wire_off[r] = r == me ? me * p.seg_wire
                                    : p.scratch_off + res.off + (r < me ? r : r - 1) * p.seg_wire;
    } else if (res.space == Space::TMP) {
        p.finish = QuantFinish::SUM2;
        p.nwires = 2;
        p.wire_off[0] = p.scratch_off + res.off;
        p.wire_off[1] = me * p.seg_wire;
    } else {
        p.wire_off[0] = res.off;
    }
    // Two-shot allreduce: the one SUMQ step's wire table. The arrival slots
    // are the TMP receives before it, one per peer, of the own range's size.
    for (const Step& st : sch.steps) {
        if (st.local != Step::LocalOp::SUMQ) continue;
        MLSL_CHECK(p.sumq_nwires == 0 && nseg == 1 && sch.fan_in == 0 &&
                       st.local_src.space == Space::TMP && st.local_dst.space != Space::TMP,
                   "a SUMQ step belongs to a two-shot allreduce, once");
        size_t slots = 0;
        for (const Step& a : sch.steps)
            if (a.phase < st.phase && a.recv_peer >= 0 && a.recv.space == Space::TMP) {
                MLSL_CHECK(a.recv.bytes == st.local_dst.bytes,
                           "two-shot arrival slots have the own range's size");
                ++slots;
            }
        MLSL_CHECK(slots + 1 <= static_cast<size_t>(kQuantRsDirectMaxRanks) && me <= slots &&
                       slots * st.local_dst.bytes == st.local_src.bytes,
                   "two-shot requantize takes one wire per rank, 8 at the most");
        const size_t units = (count + p.block - 1) / p.block;
        const size_t unit_bytes = units ? sch.wire_bytes / units : 0;
        p.sumq_nwires = static_cast<int>(slots + 1);
        p.sumq_dst_off = st.local_dst.off;
        p.sumq_units = unit_bytes ? st.local_dst.bytes / unit_bytes : 0;
        for (size_t r = 0; r <= slots; ++r)
            p.sumq_wire_off[r] =
                r == me ? st.local_dst.off
                        : p.scratch_off + st.local_src.off +
                              (r < me ? r : r - 1) * st.local_dst.bytes;
    }
    return p;
}

}  // namespace mlsl
