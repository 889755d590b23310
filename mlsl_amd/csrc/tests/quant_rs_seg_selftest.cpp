// Pure-host test of the reduce-scatter prologue over a list of tensors, built
// with ASan/UBSan and run by pytest (tests/test_quant_rs_seg_cpu.py):
//   - HostQuantizeGatherShards over the shapes of the issue (shard boundaries
//     inside tensors, on their edges and one past them, a partly and a wholly
//     padded shard), every tensor a heap allocation of exactly its size and
//     the wire and the residual exactly sized too: one element too far, or one
//     read through the table for a padding element, is an ASan report. Wire
//     and residual equal HostQuantize's, shard by shard, on the materialised
//     V' (the concatenation followed by zeros); the bytes between two shards'
//     wires are left alone;
//   - worlds 1 to 9 (direct: to 8), f32 and bf16: the prologue -> the ring or
//     the direct schedule walked by hand inside one buffer of exactly
//     plan.bytes per rank -> the SUM2 / SUMN finish into recv, three starts
//     with the residual carried and fresh tensors at every start, against the
//     same walk with HostQuantize per shard of V': plan buffers and recv
//     equal on every rank;
//   - what the twin refuses.
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
    std::vector<uint8_t> Gather() const {
        std::vector<uint8_t> v(Count() * es);
        for (size_t j = 0; j < ptrs.size(); ++j)
            std::memcpy(v.data() + offs[j] * es, ptrs[j], (offs[j + 1] - offs[j]) * es);
        return v;
    }
    const void* const* CPtrs() const { return ptrs.data(); }
};

// V' of a concatenation: zeros (all bits clear in both dtypes) up to N * shard
static std::vector<uint8_t> Padded(const std::vector<uint8_t>& v, size_t elems, size_t es) {
    std::vector<uint8_t> p(v);
    p.resize(elems * es, 0);
    return p;
}

static void TestCodec(const char* name, const std::vector<size_t>& counts, size_t N,
                      size_t shard, size_t block, DataType dt, bool use_err, size_t gap) {
    const size_t es = dt == DataType::F32 ? 4 : 2;
    TensorList tl(counts, es);
    const size_t total = tl.Count(), sw = QuantWireBytes(shard, block), stride = sw + gap;
    const std::vector<uint8_t> v = MakeInput(total, block, dt, 99u + static_cast<uint32_t>(total));
    const std::vector<uint8_t> vp = Padded(v, N * shard, es);
    // a small non-zero residual on the tensors' elements, +0 on the padding
    std::vector<uint8_t> err0(N * shard * es, 0);
    for (size_t i = 0; i < total; ++i)
        PutElem(&err0[i * es], 0.01f * static_cast<float>(static_cast<int>(i % 13) - 6), dt);
    tl.Scatter(v);
    // exactly sized: a store past either is an ASan report
    std::vector<uint8_t> wire((N - 1) * stride + sw, 0xAB), err(err0), f_wire(wire),
        f_err(err0);
    HostQuantizeGatherShards(tl.CPtrs(), tl.offs.data(), counts.size(),
                             use_err ? err.data() : nullptr, wire.data(), total, N, shard,
                             stride, block, dt, use_err);
    for (size_t j = 0; j < N; ++j)
        HostQuantize(vp.data() + j * shard * es,
                     use_err ? f_err.data() + j * shard * es : nullptr,
                     f_wire.data() + j * stride, shard, block, dt, use_err);
    EXPECT(wire == f_wire, "%s N %zu shard %zu block %zu es %zu err %d gap %zu: wire differs "
           "from HostQuantize's on V'", name, N, shard, block, es, use_err, gap);
    EXPECT(err == f_err, "%s N %zu shard %zu block %zu es %zu err %d: residual differs", name,
           N, shard, block, es, use_err);
    EXPECT(tl.Gather() == v, "%s: the prologue wrote to a tensor", name);
    for (size_t i = total * es; i < err.size(); ++i)
        if (err[i] != 0) {
            EXPECT(false, "%s N %zu shard %zu: a padding residual is not +0", name, N, shard);
            break;
        }
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
                if (st.local == Step::LocalOp::COPY)
                    std::memmove(At(buf[r], p, st.local_dst), At(buf[r], p, st.local_src),
                                 st.local_src.bytes);
                else if (st.local_dst.bytes)
                    HostQuantAccum(At(buf[r], p, st.local_dst), At(buf[r], p, st.local_src),
                                   st.local_dst.bytes / (block + 8) * block, block);
            }
    }
}

// the plan's finish into `recv` (shard elements)
static void Finish(const QuantPlan& p, const std::vector<uint8_t>& buf, uint8_t* recv,
                   DataType dt) {
    const void* wires[kQuantRsDirectMaxRanks];
    FinishWires(p, buf.data(), wires);
    switch (p.finish) {
        case QuantFinish::SUMN:
            HostQuantSumDequantN(wires, p.nwires, recv, p.count, p.block, dt);
            break;
        case QuantFinish::SUM2:
            HostQuantSumDequant(wires[0], wires[1], recv, p.count, p.block, dt);
            break;
        case QuantFinish::DEQUANT:
            HostDequantize(wires[0], recv, p.count, p.block, dt);
            break;
        default:
            EXPECT(false, "unexpected finish");
    }
}

static void TestExchange(int N, bool direct, const std::vector<size_t>& counts, size_t shard,
                         size_t block, DataType dt) {
    const size_t es = dt == DataType::F32 ? 4 : 2;
    size_t total = 0;
    for (size_t n : counts) total += n;
    const size_t n_ranks = static_cast<size_t>(N);
    if (shard == 0) shard = (total + n_ranks - 1) / n_ranks;
    const size_t units = (shard + block - 1) / block, U = block + 8;
    std::vector<Schedule> sch(N);
    std::vector<QuantPlan> plan(N);
    // segmented and flat universes: exactly plan.bytes each, residual zeroed
    std::vector<std::vector<uint8_t>> seg(N), flat(N);
    for (int r = 0; r < N; ++r) {
        sch[r] = direct ? BuildReduceScatterDirectUnits(r, N, units, U, block)
                        : BuildReduceScatterUnits(r, N, units, U, block);
        // the flat reduce-scatter's arguments, unchanged
        plan[r] = MakeQuantPlan(sch[r], n_ranks, r, shard, es);
        const QuantFinish want = N == 1   ? QuantFinish::DEQUANT
                                 : direct ? QuantFinish::SUMN
                                          : QuantFinish::SUM2;
        EXPECT(plan[r].nseg == n_ranks && plan[r].send_seg == 0 && plan[r].residual &&
                   plan[r].finish == want && plan[r].seg_wire == units * U &&
                   plan[r].seg_bytes == shard * es,
               "N=%d r=%d: not the flat reduce-scatter's plan", N, r);
        seg[r].assign(plan[r].bytes, 0);
        flat[r].assign(plan[r].bytes, 0);
    }
    for (int start = 0; start < 3; ++start) {
        for (int r = 0; r < N; ++r) {
            const QuantPlan& p = plan[r];
            const std::vector<uint8_t> in = MakeInput(total, block, dt, 1000u * (start + 1) + r);
            const std::vector<uint8_t> vp = Padded(in, n_ranks * shard, es);
            // fresh allocations at every start, as zero_grad(set_to_none) gives
            TensorList tl(counts, es);
            tl.Scatter(in);
            HostQuantizeGatherShards(tl.CPtrs(), tl.offs.data(), counts.size(),
                                     seg[r].data() + p.err_off,
                                     seg[r].data() + p.send_seg * p.seg_wire, total, p.nseg,
                                     p.count, p.seg_wire, p.block, dt, true);
            for (size_t j = 0; j < p.nseg; ++j)
                HostQuantize(vp.data() + j * p.seg_bytes,
                             flat[r].data() + p.err_off + j * p.seg_bytes,
                             flat[r].data() + (p.send_seg + j) * p.seg_wire, p.count, p.block,
                             dt, true);
            EXPECT(seg[r] == flat[r], "N=%d direct=%d r=%d start %d: prologue differs", N, direct,
                   r, start);
            EXPECT(tl.Gather() == in, "N=%d r=%d: the prologue wrote to a tensor", N, r);
        }
        Walk(sch, plan, seg, block);
        Walk(sch, plan, flat, block);
        for (int r = 0; r < N; ++r) {
            EXPECT(seg[r] == flat[r], "N=%d direct=%d r=%d start %d: plan buffers differ", N,
                   direct, r, start);
            // exactly shard elements: the finish may not write past them
            std::vector<uint8_t> recv(shard * es, 0xCD), f_recv(shard * es, 0xCD);
            Finish(plan[r], seg[r], recv.data(), dt);
            Finish(plan[r], flat[r], f_recv.data(), dt);
            EXPECT(recv == f_recv, "N=%d direct=%d r=%d start %d es %zu: recv differs", N, direct,
                   r, start, es);
        }
    }
}

static void TestRejects() {
    std::vector<float> a(8, 1.f), b(8, 2.f);
    std::vector<uint8_t> wire(2 * QuantWireBytes(8, 8), 0xAB);
    void* ptrs[2] = {a.data(), b.data()};
    const uint64_t good[3] = {0, 8, 16}, empty[3] = {0, 8, 8}, shifted[3] = {1, 8, 16};
    auto throws = [&](const uint64_t* offs, size_t nseg, size_t total, size_t nshards,
                      size_t shard, size_t stride, size_t block, DataType dt) {
        try {
            HostQuantizeGatherShards(ptrs, offs, nseg, nullptr, wire.data(), total, nshards,
                                     shard, stride, block, dt, false);
        } catch (const std::exception&) {
            return true;
        }
        return false;
    };
    const size_t sw = QuantWireBytes(8, 8);
    EXPECT(throws(empty, 2, 8, 2, 8, sw, 8, DataType::F32), "a zero count accepted");
    EXPECT(throws(good, 0, 16, 2, 8, sw, 8, DataType::F32), "nseg == 0 accepted");
    EXPECT(throws(shifted, 2, 16, 2, 8, sw, 8, DataType::F32), "offsets from 1 accepted");
    EXPECT(throws(good, 2, 15, 2, 8, sw, 8, DataType::F32), "offsets past total accepted");
    EXPECT(throws(good, 2, 16, 2, 7, sw, 8, DataType::F32), "shard * nshards < total accepted");
    EXPECT(throws(good, 2, 16, 0, 8, sw, 8, DataType::F32), "nshards == 0 accepted");
    EXPECT(throws(good, 2, 16, 2, 8, sw - 8, 8, DataType::F32), "a short wire_stride accepted");
    EXPECT(throws(good, 2, 16, 2, 8, sw + 2, 8, DataType::F32), "wire_stride + 2 accepted");
    EXPECT(throws(good, 2, 16, 2, 8, sw, 8, DataType::F64), "f64 accepted");
    EXPECT(throws(good, 2, 16, 2, 8, sw, 6, DataType::F32), "block 6 accepted");
    EXPECT(throws(good, 2, 16, 2, 8, sw, 0, DataType::F32), "block 0 accepted");
    bool no_err = false;
    try {
        HostQuantizeGatherShards(ptrs, good, 2, nullptr, wire.data(), 16, 2, 8, sw, 8,
                                 DataType::F32, true);
    } catch (const std::exception&) {
        no_err = true;
    }
    EXPECT(no_err, "use_err without err accepted");
    EXPECT(wire == std::vector<uint8_t>(wire.size(), 0xAB) && a == std::vector<float>(8, 1.f) &&
               b == std::vector<float>(8, 2.f), "a rejected call wrote");
    EXPECT(!throws(good, 2, 16, 2, 8, sw, 8, DataType::F32), "a good call rejected");
}

int main() {
    std::vector<size_t> tiny700;
    for (size_t i = 0; i < 700; ++i) tiny700.push_back(1 + i % 3);
    const std::vector<size_t> edges = {1, 255, 1, 256, 257, 3, 511};
    const struct {
        const char* name;
        std::vector<size_t> counts;
        size_t N, shard;
    } cases[] = {{"fastslow", {768, 5, 5, 5, 1024, 7}, 2, 907},
                 {"edges", edges, 3, 428},
                 {"edges", edges, 5, 257},
                 {"edges", edges, 2, 770},
                 {"edges", edges, 4, 513},
                 {"tiny700", tiny700, 8, 175},
                 {"one", {1000}, 1, 1000}};
    for (const auto& c : cases)
        for (size_t block : {256, 128})
            for (DataType dt : {DataType::F32, DataType::BF16})
                for (bool use_err : {true, false})
                    for (size_t gap : {0, 4, 8})
                        TestCodec(c.name, c.counts, c.N, c.shard, block, dt, use_err, gap);
    for (int N = 1; N <= 9; ++N)
        for (DataType dt : {DataType::F32, DataType::BF16})
            for (bool direct : {false, true}) {
                if (direct && N > 8) continue;
                TestExchange(N, direct, edges, 0, 256, dt);
                TestExchange(N, direct, {7, 300, 1, 695}, 0, 128, dt);
                // the shard given, and larger than it has to be
                TestExchange(N, direct, edges, 1284 / N + 130, 256, dt);
                // one rank and more own nothing but padding
                TestExchange(N, direct, {2, 3}, 0, 8, dt);
            }
    for (DataType dt : {DataType::F32, DataType::BF16})
        for (bool direct : {false, true}) {
            TestExchange(3, direct, edges, 428, 256, dt);
            TestExchange(5, direct, edges, 257, 256, dt);
            TestExchange(2, direct, edges, 770, 256, dt);
            TestExchange(4, direct, edges, 513, 256, dt);
        }
    TestRejects();
    if (g_failures) {
        std::printf("%d FAILURES\n", g_failures);
        return 1;
    }
    std::printf("quant_rs_seg_selftest: all passed\n");
    return 0;
}
