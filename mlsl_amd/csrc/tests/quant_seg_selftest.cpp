// Pure-host test of the codec over a list of tensors, built with ASan/UBSan
// and run by pytest (tests/test_quant_seg_cpu.py):
//   - HostQuantizeGather / HostDequantizeScatter over the segment layouts of
//     tests/quant_seg_ref.py, every tensor a heap allocation of exactly its
//     size, the wire and the residual exactly sized too: one element too far
//     is an ASan report.
//     Wire and residual equal HostQuantize's on the concatenation; the
//     tensors equal (q * scale) * post_scale written out here, with and
//     without round_first, and HostDequantize's bytes at post_scale 1;
//   - worlds 1 to 9 (two-shot: to 8), f32 and bf16: gather -> the ring or the
//     two-shot schedule walked by hand inside one buffer of exactly
//     plan.bytes per rank -> scatter, three starts with the residual carried,
//     against the same walk with HostQuantize / HostDequantize on the
//     concatenation: equal on all ranks, and equal to the flat result's
//     stored elements times post_scale (the finish runs with round_first);
//   - what the twins refuse.
// Exit 0 = PASS.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../comm/quant.hpp"
#include "../comm/quant_plan.hpp"
#include "../comm/schedule.hpp"

using namespace mlsl;

static int g_failures = 0;

#define EXPECT(cond, ...)                                                     \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__);                  \
            std::printf(__VA_ARGS__);                                         \
            std::printf("\n");                                                \
            ++g_failures;                                                     \
        }                                                                     \
    } while (0)

static uint16_t ToBf16(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1);
    return static_cast<uint16_t>(u >> 16);
}

static void PutElem(uint8_t* p, float v, DataType dt) {
    if (dt == DataType::F32) {
        std::memcpy(p, &v, 4);
    } else {
        const uint16_t h = ToBf16(v);
        std::memcpy(p, &h, 2);
    }
}

// `count` elements in dt storage: block 0 is rounding ties under a scale of
// 2^-3, block 1 is zero, the rest pseudo-random
static std::vector<uint8_t> MakeInput(size_t count, size_t block, DataType dt, uint32_t seed) {
    const size_t es = dt == DataType::F32 ? 4 : 2;
    std::vector<uint8_t> in(count * es);
    uint32_t lcg = seed;
    for (size_t i = 0; i < count; ++i) {
        lcg = lcg * 1664525u + 1013904223u;
        float v = (static_cast<float>(lcg >> 8) / 8388608.f - 1.f) * 3.f;
        if (i < block) v = i == 0 ? 127 * 0.125f : (static_cast<float>(i % 127) + 0.5f) * 0.125f;
        else if (i < 2 * block) v = 0.f;
        PutElem(&in[i * es], v, dt);
    }
    return in;
}

// A list of tensors, each its own allocation of exactly counts[j] elements.
struct TensorList {
    std::vector<std::unique_ptr<uint8_t[]>> mem;
    std::vector<void*> ptrs;
    std::vector<uint64_t> offs;
    size_t es;
    TensorList(const std::vector<size_t>& counts, size_t elem_size) : offs(1, 0), es(elem_size) {
        for (size_t n : counts) {
            mem.emplace_back(new uint8_t[n * es]);
            ptrs.push_back(mem.back().get());
            offs.push_back(offs.back() + n);
        }
    }
    size_t Count() const { return static_cast<size_t>(offs.back()); }
    void Scatter(const std::vector<uint8_t>& v) {
        for (size_t j = 0; j < ptrs.size(); ++j)
            std::memcpy(ptrs[j], v.data() + offs[j] * es, (offs[j + 1] - offs[j]) * es);
    }
    void Fill(uint8_t b) {
        for (size_t j = 0; j < ptrs.size(); ++j)
            std::memset(ptrs[j], b, (offs[j + 1] - offs[j]) * es);
    }
    std::vector<uint8_t> Gather() const {
        std::vector<uint8_t> v(Count() * es);
        for (size_t j = 0; j < ptrs.size(); ++j)
            std::memcpy(v.data() + offs[j] * es, ptrs[j], (offs[j + 1] - offs[j]) * es);
        return v;
    }
    const void* const* CPtrs() const { return ptrs.data(); }
};

static float FromBf16(uint16_t h) {
    const uint32_t u = static_cast<uint32_t>(h) << 16;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

// (q * scale) * post_scale from the wire, written out; round_first: q * scale
// goes through bf16 before it is scaled (bf16 only)
static std::vector<uint8_t> WantScatter(const std::vector<uint8_t>& wire, size_t count,
                                        size_t block, DataType dt, float post_scale,
                                        bool round_first = false) {
    const size_t es = dt == DataType::F32 ? 4 : 2;
    std::vector<uint8_t> out(count * es);
    for (size_t i = 0; i < count; ++i) {
        const uint8_t* wb = wire.data() + (i / block) * (block + 8);
        float scale;
        std::memcpy(&scale, wb, 4);
        float dq = static_cast<float>(static_cast<int8_t>(wb[8 + i % block])) * scale;
        if (round_first && dt == DataType::BF16) dq = FromBf16(ToBf16(dq));
        PutElem(&out[i * es], dq * post_scale, dt);
    }
    return out;
}

static void TestCodec(const char* name, const std::vector<size_t>& counts, size_t block,
                      DataType dt, bool use_err) {
    const size_t es = dt == DataType::F32 ? 4 : 2;
    TensorList tl(counts, es);
    const size_t count = tl.Count(), wbytes = QuantWireBytes(count, block);
    const std::vector<uint8_t> v = MakeInput(count, block, dt, 99u + static_cast<uint32_t>(count));
    std::vector<uint8_t> err0 = MakeInput(count, block, dt, 5u);
    for (size_t i = 0; i < count; ++i) {   // a small non-zero residual
        float e = 0.01f * static_cast<float>(static_cast<int>(i % 13) - 6);
        PutElem(&err0[i * es], e, dt);
    }
    tl.Scatter(v);
    // exactly sized: a store past either is an ASan report
    std::vector<uint8_t> wire(wbytes, 0xAB), err(err0), f_wire(wbytes, 0xAB), f_err(err0);
    HostQuantizeGather(tl.CPtrs(), tl.offs.data(), counts.size(), use_err ? err.data() : nullptr,
                       wire.data(), count, block, dt, use_err);
    HostQuantize(v.data(), use_err ? f_err.data() : nullptr, f_wire.data(), count, block, dt,
                 use_err);
    EXPECT(wire == f_wire, "%s block %zu es %zu err %d: wire differs from HostQuantize's", name,
           block, es, use_err);
    EXPECT(err == f_err, "%s block %zu es %zu err %d: residual differs", name, block, es,
           use_err);
    EXPECT(tl.Gather() == v, "%s: the gather wrote to a tensor", name);
    float s0, s1;
    std::memcpy(&s0, wire.data(), 4);
    std::memcpy(&s1, wire.data() + block + 8, 4);
    EXPECT(use_err || (s0 == 0.125f && s1 == 1.f), "%s: tie/zero block scales %g %g", name, s0,
           s1);

    std::vector<uint8_t> flat(count * es, 0xCD);
    HostDequantize(wire.data(), flat.data(), count, block, dt);
    const std::vector<uint8_t> keep(wire);
    for (bool rf : {false, true})
        for (float ps : {1.0f, 0.5f, 1.0f / 3.0f}) {
            tl.Fill(0xCD);
            HostDequantizeScatter(wire.data(), tl.ptrs.data(), tl.offs.data(), counts.size(),
                                  count, block, dt, ps, rf);
            const std::vector<uint8_t> got = tl.Gather();
            EXPECT(got == WantScatter(wire, count, block, dt, ps, rf),
                   "%s block %zu es %zu post_scale %g round_first %d: scatter differs", name,
                   block, es, ps, rf);
            EXPECT(ps != 1.0f || got == flat, "%s block %zu es %zu: post_scale 1 differs from "
                   "HostDequantize", name, block, es);
        }
    EXPECT(wire == keep, "%s: the scatter wrote to the wire", name);
}

// where a BufRef of a rank's schedule lives inside its plan-sized buffer
static uint8_t* At(std::vector<uint8_t>& buf, const QuantPlan& p, const BufRef& b) {
    return buf.data() + (b.space == Space::TMP ? p.scratch_off : 0) + b.off;
}

// Every phase: each send lands where the receiver's step of the same phase
// points, then the phase's local ops run.
static void Walk(const std::vector<Schedule>& sch, const std::vector<QuantPlan>& plan,
                 std::vector<std::vector<uint8_t>>& buf, size_t block) {
    const int N = static_cast<int>(sch.size());
    for (int phase = 0; phase < sch[0].num_phases; ++phase) {
        for (int r = 0; r < N; ++r)
            for (const Step& st : sch[r].steps) {
                if (st.phase != phase || st.send_peer < 0 || st.send.bytes == 0) continue;
                const int to = st.send_peer;
                for (const Step& pt : sch[to].steps)
                    if (pt.phase == phase && pt.recv_peer == r)
                        std::memcpy(At(buf[to], plan[to], pt.recv), At(buf[r], plan[r], st.send),
                                    st.send.bytes);
            }
        for (int r = 0; r < N; ++r)
            for (const Step& st : sch[r].steps) {
                if (st.phase != phase || st.local == Step::LocalOp::NONE) continue;
                const QuantPlan& p = plan[r];
                if (st.local == Step::LocalOp::SUMQ) {
                    const void* wires[kQuantRsDirectMaxRanks];
                    SumqWires(p, buf[r].data(), wires);
                    if (p.sumq_units)
                        HostQuantSumRequantN(wires, p.sumq_nwires, buf[r].data() + p.sumq_dst_off,
                                             p.sumq_units, block);
                } else if (st.local == Step::LocalOp::COPY) {
                    std::memmove(At(buf[r], p, st.local_dst), At(buf[r], p, st.local_src),
                                 st.local_src.bytes);
                } else if (st.local_dst.bytes) {
                    HostQuantAccum(At(buf[r], p, st.local_dst), At(buf[r], p, st.local_src),
                                   st.local_dst.bytes / (block + 8) * block, block);
                }
            }
    }
}

static void TestExchange(int N, bool two_shot, const std::vector<size_t>& counts, size_t block,
                         DataType dt) {
    const size_t es = dt == DataType::F32 ? 4 : 2;
    size_t count = 0;
    for (size_t n : counts) count += n;
    const size_t units = (count + block - 1) / block, U = block + 8;
    const float post_scale = 1.0f / static_cast<float>(N);
    std::vector<Schedule> sch(N);
    std::vector<QuantPlan> plan(N);
    // segmented and flat universes: exactly plan.bytes each, residual zeroed
    std::vector<std::vector<uint8_t>> seg(N), flat(N);
    for (int r = 0; r < N; ++r) {
        sch[r] = two_shot ? BuildAllReduceTwoShotUnits(r, N, units, U, block)
                          : BuildAllReduceRingUnits(r, N, units, U, block);
        plan[r] = MakeQuantPlan(sch[r], 1, r, count, es);
        EXPECT(plan[r].nseg == 1 && plan[r].send_seg == 0 && plan[r].residual &&
                   plan[r].finish == QuantFinish::DEQUANT,
               "N=%d r=%d: not the flat allreduce's plan", N, r);
        seg[r].assign(plan[r].bytes, 0);
        flat[r].assign(plan[r].bytes, 0);
    }
    for (int start = 0; start < 3; ++start) {
        std::vector<TensorList> tls;
        std::vector<std::vector<uint8_t>> in(N);
        for (int r = 0; r < N; ++r) {
            const QuantPlan& p = plan[r];
            in[r] = MakeInput(count, block, dt, 1000u * (start + 1) + r);
            // fresh allocations at every start, as zero_grad(set_to_none) gives
            tls.emplace_back(counts, es);
            tls.back().Scatter(in[r]);
            HostQuantizeGather(tls.back().CPtrs(), tls.back().offs.data(), counts.size(),
                               seg[r].data() + p.err_off, seg[r].data(), p.count, p.block, dt,
                               true);
            HostQuantize(in[r].data(), flat[r].data() + p.err_off, flat[r].data(), p.count,
                         p.block, dt, true);
        }
        Walk(sch, plan, seg, block);
        Walk(sch, plan, flat, block);
        for (int r = 0; r < N; ++r) {
            const QuantPlan& p = plan[r];
            EXPECT(seg[r] == flat[r], "N=%d two_shot=%d r=%d start %d: plan buffers differ", N,
                   two_shot, r, start);
            HostDequantizeScatter(seg[r].data() + p.wire_off[0], tls[r].ptrs.data(),
                                  tls[r].offs.data(), counts.size(), count, block, dt,
                                  post_scale, /*round_first=*/true);
            const std::vector<uint8_t> wire(flat[r].begin() + p.wire_off[0],
                                            flat[r].begin() + p.wire_off[0] + units * U);
            // the flat finish's elements, scaled: what the request computes
            std::vector<uint8_t> scaled(count * es);
            HostDequantize(wire.data(), scaled.data(), count, block, dt);
            for (size_t i = 0; i < count; ++i) {
                float v;
                if (dt == DataType::F32) {
                    std::memcpy(&v, &scaled[i * 4], 4);
                } else {
                    uint16_t h;
                    std::memcpy(&h, &scaled[i * 2], 2);
                    v = FromBf16(h);
                }
                PutElem(&scaled[i * es], v * post_scale, dt);
            }
            EXPECT(tls[r].Gather() == scaled,
                   "N=%d two_shot=%d r=%d start %d es %zu: not the flat result scaled", N,
                   two_shot, r, start, es);
            EXPECT(tls[r].Gather() == WantScatter(wire, count, block, dt, post_scale, true),
                   "N=%d two_shot=%d r=%d start %d es %zu: result differs", N, two_shot, r,
                   start, es);
            EXPECT(tls[r].Gather() == tls[0].Gather(),
                   "N=%d two_shot=%d r=%d start %d: differs from rank 0", N, two_shot, r, start);
        }
    }
}

static void TestRejects() {
    std::vector<float> a(8, 1.f), b(8, 2.f);
    std::vector<uint8_t> wire(QuantWireBytes(16, 8), 0xAB);
    void* ptrs[2] = {a.data(), b.data()};
    const uint64_t good[3] = {0, 8, 16}, empty[3] = {0, 8, 8}, shifted[3] = {1, 8, 16},
                   lessthan[3] = {0, 8, 15};
    auto throws = [&](const uint64_t* offs, size_t nseg, size_t block, DataType dt) {
        int n = 0;
        try {
            HostQuantizeGather(ptrs, offs, nseg, nullptr, wire.data(), 16, block, dt, false);
        } catch (const std::exception&) {
            ++n;
        }
        try {
            HostDequantizeScatter(wire.data(), ptrs, offs, nseg, 16, block, dt, 1.f);
        } catch (const std::exception&) {
            ++n;
        }
        return n;
    };
    EXPECT(throws(empty, 2, 8, DataType::F32) == 2, "a zero count accepted");
    EXPECT(throws(good, 0, 8, DataType::F32) == 2, "nseg == 0 accepted");
    EXPECT(throws(shifted, 2, 8, DataType::F32) == 2, "offsets from 1 accepted");
    EXPECT(throws(lessthan, 2, 8, DataType::F32) == 2, "offsets short of count accepted");
    EXPECT(throws(good, 2, 8, DataType::F64) == 2, "f64 accepted");
    EXPECT(throws(good, 2, 6, DataType::F32) == 2, "block 6 accepted");
    EXPECT(throws(good, 2, 0, DataType::F32) == 2, "block 0 accepted");
    EXPECT(wire == std::vector<uint8_t>(wire.size(), 0xAB) && a == std::vector<float>(8, 1.f) &&
               b == std::vector<float>(8, 2.f), "a rejected call wrote");
    EXPECT(throws(good, 2, 8, DataType::F32) == 0, "a good call rejected");
}

int main() {
    std::vector<size_t> tiny700, big(22, 100003);
    for (size_t i = 0; i < 700; ++i) tiny700.push_back(1 + i % 3);
    const struct {
        const char* name;
        std::vector<size_t> counts;
    } layouts[] = {{"one", {1000}},
                   {"edges", {1, 255, 1, 256, 257, 3, 511}},
                   {"tiny700", tiny700},
                   {"fastslow", {768, 5, 5, 5, 1024, 7}},
                   {"big", big}};
    for (const auto& l : layouts)
        for (size_t block : {256, 128})
            for (DataType dt : {DataType::F32, DataType::BF16})
                for (bool use_err : {true, false}) TestCodec(l.name, l.counts, block, dt, use_err);
    for (int N = 1; N <= 9; ++N)
        for (DataType dt : {DataType::F32, DataType::BF16}) {
            TestExchange(N, false, {1, 255, 1, 256, 257, 3, 511}, 256, dt);
            TestExchange(N, false, {7, 300, 1, 695}, 128, dt);
            if (N <= 8) {
                TestExchange(N, true, {1, 255, 1, 256, 257, 3, 511}, 256, dt);
                TestExchange(N, true, {7, 300, 1, 695}, 128, dt);
            }
        }
    TestRejects();
    if (g_failures) {
        std::printf("%d FAILURES\n", g_failures);
        return 1;
    }
    std::printf("quant_seg_selftest: all passed\n");
    return 0;
}
