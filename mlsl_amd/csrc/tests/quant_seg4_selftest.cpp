// Pure-host test of the int4 codec over a list of tensors, built with
// ASan/UBSan and run by pytest (tests/test_quant_seg4_cpu.py):
//   - HostQuantizeGather / HostDequantizeScatter at bits = 4 over `edges` and
//     `tiny700`, blocks 256 and 24, every tensor, the wire and the residual a
//     heap allocation of exactly its size: one element too far is an ASan
//     report. Wire and residual equal HostQuantize's on the concatenation, the
//     tensors HostDequantize's at post_scale 1;
//   - worlds 1 to 8: gather -> the two-shot schedule walked by hand inside one
//     buffer of exactly plan.bytes per rank -> scatter, three starts with the
//     residual carried, against the same walk with the flat twins.
// Exit 0 = PASS.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../comm/quant.hpp"
#include "../comm/quant_plan.hpp"
#include "../comm/schedule.hpp"

using namespace mlsl;
using Bytes = std::vector<uint8_t>;

static int g_failures = 0;
#define EXPECT(cond, ...)                                                              \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            std::printf("FAIL line %d: ", __LINE__);                                   \
            std::printf(__VA_ARGS__);                                                  \
            std::printf("\n");                                                         \
            ++g_failures;                                                              \
        }                                                                              \
    } while (0)

// `count` pseudo-random elements of magnitude `amp` in dt storage (bf16 by
// truncation: any bf16 value will do)
static Bytes MakeInput(size_t count, DataType dt, uint32_t seed, float amp = 3.f) {
    const size_t es = dt == DataType::F32 ? 4 : 2;
    Bytes in(count * es);
    uint32_t lcg = seed;
    for (size_t i = 0; i < count; ++i) {
        lcg = lcg * 1664525u + 1013904223u;
        const float v = (static_cast<float>(lcg >> 8) / 8388608.f - 1.f) * amp;
        std::memcpy(&in[i * es], reinterpret_cast<const uint8_t*>(&v) + (4 - es), es);
    }
    return in;
}

// A list of tensors, each its own allocation of exactly counts[j] elements.
struct TensorList {
    std::vector<std::unique_ptr<uint8_t[]>> mem;
    std::vector<void*> ptrs;
    std::vector<uint64_t> offs{0};
    size_t es;
    TensorList(const std::vector<size_t>& counts, size_t elem_size, const Bytes& v)
        : es(elem_size) {
        for (size_t n : counts) {
            mem.emplace_back(new uint8_t[n * es]);
            std::memcpy(mem.back().get(), v.data() + offs.back() * es, n * es);
            ptrs.push_back(mem.back().get());
            offs.push_back(offs.back() + n);
        }
    }
    Bytes Gather() const {
        Bytes v(offs.back() * es);
        for (size_t j = 0; j < ptrs.size(); ++j)
            std::memcpy(v.data() + offs[j] * es, ptrs[j], (offs[j + 1] - offs[j]) * es);
        return v;
    }
};

static void TestCodec(const std::vector<size_t>& counts, size_t block, DataType dt,
                      bool use_err) {
    const size_t es = dt == DataType::F32 ? 4 : 2;
    size_t count = 0;
    for (size_t n : counts) count += n;
    const size_t wbytes = QuantWireBytes(count, block, 4);
    const Bytes v = MakeInput(count, dt, 99u + static_cast<uint32_t>(count));
    TensorList tl(counts, es, v);
    Bytes wire(wbytes, 0xAB), f_wire(wbytes, 0xAB);
    Bytes err = MakeInput(count, dt, 5u, 0.01f), f_err(err);
    HostQuantizeGather(tl.ptrs.data(), tl.offs.data(), counts.size(),
                       use_err ? err.data() : nullptr, wire.data(), count, block, dt, use_err, 4);
    HostQuantize(v.data(), use_err ? f_err.data() : nullptr, f_wire.data(), count, block, dt,
                 use_err, 4);
    EXPECT(wire == f_wire && err == f_err && tl.Gather() == v,
           "gather: %zu tensors block %zu es %zu err %d", counts.size(), block, es, use_err);
    Bytes flat(count * es, 0xCD);
    HostDequantize(wire.data(), flat.data(), count, block, dt, 4);
    HostDequantizeScatter(wire.data(), tl.ptrs.data(), tl.offs.data(), counts.size(), count,
                          block, dt, 1.f, /*round_first=*/true, 4);
    EXPECT(tl.Gather() == flat && wire == f_wire, "scatter: %zu tensors block %zu es %zu",
           counts.size(), block, es);
}

static uint8_t* At(Bytes& buf, const QuantPlan& p, const BufRef& b) {
    return buf.data() + (b.space == Space::TMP ? p.scratch_off : 0) + b.off;
}

// Every phase: each send lands where the receiver's step of the same phase
// points, then the owners sum and requantize.
static void Walk(const std::vector<Schedule>& sch, const std::vector<QuantPlan>& plan,
                 std::vector<Bytes>& buf, size_t block) {
    const int N = static_cast<int>(sch.size());
    for (int phase = 0; phase < sch[0].num_phases; ++phase) {
        for (int r = 0; r < N; ++r)
            for (const Step& st : sch[r].steps) {
                if (st.phase != phase || st.send_peer < 0 || st.send.bytes == 0) continue;
                for (const Step& pt : sch[st.send_peer].steps)
                    if (pt.phase == phase && pt.recv_peer == r)
                        std::memcpy(At(buf[st.send_peer], plan[st.send_peer], pt.recv),
                                    At(buf[r], plan[r], st.send), st.send.bytes);
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
                                             p.sumq_units, block, 4);
                } else {
                    EXPECT(st.local == Step::LocalOp::COPY, "two-shot: an accumulate step");
                    std::memmove(At(buf[r], p, st.local_dst), At(buf[r], p, st.local_src),
                                 st.local_src.bytes);
                }
            }
    }
}

static void TestExchange(int N, const std::vector<size_t>& counts, size_t block, DataType dt) {
    const size_t es = dt == DataType::F32 ? 4 : 2;
    size_t count = 0;
    for (size_t n : counts) count += n;
    const size_t units = (count + block - 1) / block, U = block / 2 + 8;
    std::vector<Schedule> sch(N);
    std::vector<QuantPlan> plan(N);
    std::vector<Bytes> seg(N), flat(N);
    for (int r = 0; r < N; ++r) {
        sch[r] = BuildAllReduceTwoShotUnits(r, N, units, U, block);
        plan[r] = MakeQuantPlan(sch[r], 1, r, count, es, QuantGather::NONE, 4);
        EXPECT(plan[r].bits == 4 && plan[r].seg_wire == units * U &&
                   plan[r].finish == QuantFinish::DEQUANT,
               "N=%d r=%d: plan not sized at block / 2 + 8 per block", N, r);
        seg[r].assign(plan[r].bytes, 0);
        flat[r].assign(plan[r].bytes, 0);
    }
    for (int start = 0; start < 3; ++start) {
        std::vector<TensorList> tls;
        for (int r = 0; r < N; ++r) {
            const QuantPlan& p = plan[r];
            const Bytes in = MakeInput(count, dt, 1000u * (start + 1) + r);
            tls.emplace_back(counts, es, in);   // fresh allocations at every start
            HostQuantizeGather(tls[r].ptrs.data(), tls[r].offs.data(), counts.size(),
                               seg[r].data() + p.err_off, seg[r].data(), count, block, dt, true, 4);
            HostQuantize(in.data(), flat[r].data() + p.err_off, flat[r].data(), count, block, dt,
                         true, 4);
        }
        Walk(sch, plan, seg, block);
        Walk(sch, plan, flat, block);
        for (int r = 0; r < N; ++r) {
            const QuantPlan& p = plan[r];
            EXPECT(seg[r] == flat[r], "N=%d r=%d start %d: plan buffers differ", N, r, start);
            Bytes want(count * es);
            HostDequantize(flat[r].data() + p.wire_off[0], want.data(), count, block, dt, 4);
            HostDequantizeScatter(seg[r].data() + p.wire_off[0], tls[r].ptrs.data(),
                                  tls[r].offs.data(), counts.size(), count, block, dt, 1.f,
                                  /*round_first=*/true, 4);
            EXPECT(tls[r].Gather() == want && tls[r].Gather() == tls[0].Gather(),
                   "N=%d r=%d start %d es %zu: result differs", N, r, start, es);
        }
    }
}

int main() {
    const std::vector<size_t> edges{1, 255, 1, 256, 257, 3, 511};
    std::vector<size_t> tiny700;
    for (size_t i = 0; i < 700; ++i) tiny700.push_back(1 + i % 3);
    for (DataType dt : {DataType::F32, DataType::BF16})
        for (size_t block : {256, 24}) {
            for (bool use_err : {true, false}) {
                TestCodec(edges, block, dt, use_err);
                TestCodec(tiny700, block, dt, use_err);
            }
            for (int N = 1; N <= 8; ++N) TestExchange(N, edges, block, dt);
        }
    if (g_failures) {
        std::printf("%d FAILURES\n", g_failures);
        return 1;
    }
    std::printf("quant_seg4_selftest: all passed\n");
    return 0;
}
