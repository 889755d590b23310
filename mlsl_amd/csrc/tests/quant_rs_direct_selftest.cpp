// Pure-host test of the one-shot (direct) quantized reduce-scatter and of
// the plan of every compressed chunk, built with ASan/UBSan and run by pytest
// (tests/test_quant_rs_direct_cpu.py):
//   - BuildReduceScatterDirectUnits for worlds 1..9: the simulator accepts
//     the schedules (every send has a matching receive of the same size),
//     the receive slots are disjoint and cover tmp_bytes, and wire segment
//     `to` goes to rank `to` and lands in the slot the epilogue reads;
//   - MakeQuantPlan for the allreduce, ring and direct reduce-scatter unit
//     schedules of worlds 1..9, every rank, against formulas written out
//     here: layout, finish and wire table;
//   - HostQuantize -> the exchange walked by hand -> HostQuantSumDequantN
//     for worlds 2..8, all inside one plan-sized buffer per rank, against the
//     sum of the dequantized wires in rank order with one fmaf per wire.
// Exit 0 = PASS.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
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

static std::vector<Schedule> Build(int N, size_t units, size_t block) {
    std::vector<Schedule> sch(N);
    for (int r = 0; r < N; ++r)
        sch[r] = BuildReduceScatterDirectUnits(r, N, units, block + 8, block);
    return sch;
}

static void TestSchedule(int N, size_t units, size_t block) {
    const size_t segB = units * (block + 8);
    std::vector<Schedule> sch = Build(N, units, block);
    for (int r = 0; r < N; ++r) {
        const Schedule& s = sch[r];
        EXPECT(s.dtype == DataType::U8 && s.quant_block == block, "N=%d r=%d header", N, r);
        EXPECT(s.wire_bytes == N * segB, "N=%d r=%d wire_bytes %zu", N, r, s.wire_bytes);
        if (N == 1) {
            EXPECT(s.steps.empty() && s.num_phases == 0 && s.tmp_bytes == 0 && s.fan_in == 0,
                   "N=1 must have no traffic");
            EXPECT(s.result.space == Space::SEND && s.result.off == 0 &&
                       s.result.bytes == segB, "N=1 result");
            continue;
        }
        EXPECT(s.steps.size() == static_cast<size_t>(N - 1) && s.num_phases == N - 1,
               "N=%d r=%d: %zu steps, %d phases", N, r, s.steps.size(), s.num_phases);
        EXPECT(s.tmp_bytes == (N - 1) * segB, "N=%d r=%d tmp_bytes %zu", N, r, s.tmp_bytes);
        EXPECT(s.fan_in == static_cast<size_t>(N - 1), "N=%d r=%d fan_in %zu", N, r, s.fan_in);
        EXPECT(s.result.space == Space::TMP && s.result.off == 0 &&
                   s.result.bytes == s.tmp_bytes, "N=%d r=%d result", N, r);
        std::vector<size_t> offs;
        std::vector<int> sent_to(N, 0), got_from(N, 0);
        for (const Step& st : s.steps) {
            EXPECT(st.local == Step::LocalOp::NONE, "N=%d r=%d: local op", N, r);
            EXPECT(st.send_peer >= 0 && st.send_peer < N && st.send_peer != r &&
                       st.recv_peer >= 0 && st.recv_peer < N && st.recv_peer != r,
                   "N=%d r=%d peers %d %d", N, r, st.send_peer, st.recv_peer);
            if (st.send_peer < 0 || st.send_peer >= N || st.recv_peer < 0 || st.recv_peer >= N)
                return;
            // segment `to` goes to rank `to`
            EXPECT(st.send.space == Space::SEND && st.send.bytes == segB &&
                       st.send.off == static_cast<size_t>(st.send_peer) * segB,
                   "N=%d r=%d: send to %d reads off %zu", N, r, st.send_peer, st.send.off);
            EXPECT(st.recv.space == Space::TMP && st.recv.bytes == segB &&
                       // ascending rank order with r left out
                       st.recv.off == (st.recv_peer - (st.recv_peer > r)) * segB,
                   "N=%d r=%d: recv from %d lands at %zu", N, r, st.recv_peer, st.recv.off);
            ++sent_to[st.send_peer];
            ++got_from[st.recv_peer];
            offs.push_back(st.recv.off);
            // the receiver expects this rank in the same phase
            bool matched = false;
            for (const Step& pt : sch[st.send_peer].steps)
                matched = matched || (pt.phase == st.phase && pt.recv_peer == r);
            EXPECT(matched, "N=%d r=%d phase %d: rank %d does not receive", N, r, st.phase,
                   st.send_peer);
        }
        for (int p = 0; p < N; ++p)
            EXPECT(sent_to[p] == (p != r) && got_from[p] == (p != r),
                   "N=%d r=%d peer %d: %d sends %d recvs", N, r, p, sent_to[p], got_from[p]);
        // disjoint slots that cover tmp_bytes
        std::sort(offs.begin(), offs.end());
        for (size_t k = 0; k < offs.size(); ++k)
            EXPECT(offs[k] == k * segB, "N=%d r=%d slot %zu at %zu", N, r, k, offs[k]);
    }
    // every send has a matching receive: the simulator throws otherwise
    std::vector<std::vector<uint8_t>> sbuf(N), rbuf(N);
    for (int r = 0; r < N; ++r) sbuf[r].assign(N * segB, static_cast<uint8_t>(r + 1));
    try {
        SimulateSchedules(sch, sbuf, rbuf);
    } catch (const std::exception& e) {
        EXPECT(false, "N=%d simulator: %s", N, e.what());
    }
}

static size_t Al16(size_t x) { return (x + 15) / 16 * 16; }

enum class Algo { ALLREDUCE, RING, DIRECT };

// Every field of every rank's plan against the layout and finish rules
// written out here (quant_plan.hpp states them; nothing below calls the plan
// for an expectation).
static void TestPlan(Algo algo, int N, size_t units, size_t block, size_t es) {
    const size_t U = block + 8, segB = units * U;
    const size_t count = units * block - 3;   // a tail block: units = ceil(count / block)
    for (int r = 0; r < N; ++r) {
        const size_t me = static_cast<size_t>(r);
        const Schedule sch =
            algo == Algo::ALLREDUCE ? BuildAllReduceRingUnits(r, N, units, U, block)
            : algo == Algo::RING    ? BuildReduceScatterUnits(r, N, units, U, block)
                                    : BuildReduceScatterDirectUnits(r, N, units, U, block);
        const size_t nseg = algo == Algo::ALLREDUCE ? 1 : static_cast<size_t>(N);
        QuantPlan p;
        bool threw = false;
        try {
            p = MakeQuantPlan(sch, nseg, me, count, es);
        } catch (const std::exception&) {
            threw = true;
        }
        const int a = static_cast<int>(algo);
        EXPECT(threw == (algo == Algo::DIRECT && N > 8), "plan algo=%d N=%d r=%d: threw=%d",
               a, N, r, threw);
        if (threw) continue;
        // scratch: the allreduce ring's largest segment, two ring slots (one
        // at world 2), one slot per peer for direct
        const size_t tmp = N == 1                 ? 0
                           : algo == Algo::ALLREDUCE ? (units + N - 1) / N * U
                           : algo == Algo::RING      ? std::min(2, N - 1) * segB
                                                     : (N - 1) * segB;
        const size_t wire_end = nseg * segB, scratch = Al16(wire_end);
        const size_t err = scratch + Al16(tmp), err_end = err + nseg * count * es;
        EXPECT(p.block == block && p.count == count && p.nseg == nseg &&
                   p.seg_bytes == count * es && p.seg_wire == segB,
               "plan algo=%d N=%d r=%d: nseg %zu seg_wire %zu", a, N, r, p.nseg, p.seg_wire);
        EXPECT(p.scratch_off == scratch && p.err_off == err && p.bytes == Al16(err_end),
               "plan algo=%d N=%d r=%d: offsets %zu %zu %zu", a, N, r, p.scratch_off,
               p.err_off, p.bytes);
        EXPECT(p.scratch_off % 16 == 0 && p.err_off % 16 == 0 && p.bytes % 16 == 0,
               "plan algo=%d N=%d r=%d: unaligned region", a, N, r);
        EXPECT(wire_end <= p.scratch_off && p.scratch_off + sch.tmp_bytes <= p.err_off &&
                   sch.tmp_bytes == tmp && err_end <= p.bytes,
               "plan algo=%d N=%d r=%d: regions overlap", a, N, r);
        std::vector<size_t> want;
        QuantFinish fin = QuantFinish::DEQUANT;
        if (algo == Algo::ALLREDUCE || N == 1) {
            want = {0};
        } else if (algo == Algo::RING) {
            fin = QuantFinish::SUM2;   // arrived partial sum first, own segment second
            want = {scratch + (N % 2) * segB, me * segB};
        } else {
            fin = QuantFinish::SUMN;   // ascending rank; peers fill the slots in that order
            for (size_t q = 0; q < nseg; ++q)
                want.push_back(q == me ? me * segB : scratch + (q - (q > me)) * segB);
        }
        EXPECT(p.finish == fin && p.nwires == static_cast<int>(want.size()),
               "plan algo=%d N=%d r=%d: finish %d nwires %d", a, N, r,
               static_cast<int>(p.finish), p.nwires);
        for (size_t k = 0; k < want.size() && k < 8; ++k) {
            EXPECT(p.wire_off[k] == want[k], "plan algo=%d N=%d r=%d: wire %zu at %zu", a, N, r,
                   k, p.wire_off[k]);
            // a whole wire inside the wire region or inside the scratch
            const size_t lo = p.wire_off[k], hi = lo + (nseg > 1 ? segB : wire_end);
            EXPECT(hi <= wire_end || (lo >= p.scratch_off && hi <= p.scratch_off + tmp),
                   "plan algo=%d N=%d r=%d: wire %zu outside its region", a, N, r, k);
        }
    }
}

static uint16_t ToBf16(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1);
    return static_cast<uint16_t>(u >> 16);
}

static void TestExchange(int N, size_t count, size_t block, DataType dt) {
    const size_t es = dt == DataType::F32 ? 4 : 2;
    const size_t units = (count + block - 1) / block;
    const size_t segB = units * (block + 8);
    std::vector<Schedule> sch = Build(N, units, block);
    // one plan-sized buffer per rank: wire, scratch and residual inside it
    std::vector<QuantPlan> plan(N);
    std::vector<std::vector<uint8_t>> buf(N);
    // inputs: a different magnitude per rank, so the block scales differ
    uint32_t lcg = 12345u + static_cast<uint32_t>(N);
    for (int r = 0; r < N; ++r) {
        std::vector<uint8_t> in(N * count * es);
        for (size_t i = 0; i < N * count; ++i) {
            lcg = lcg * 1664525u + 1013904223u;
            const float v = (static_cast<float>(lcg >> 8) / 8388608.f - 1.f) * (1.f + r);
            if (dt == DataType::F32) std::memcpy(&in[i * 4], &v, 4);
            else {
                const uint16_t h = ToBf16(v);
                std::memcpy(&in[i * 2], &h, 2);
            }
        }
        const QuantPlan& p = plan[r] = MakeQuantPlan(sch[r], N, r, count, es);
        buf[r].assign(p.bytes, 0xAB);
        std::memset(buf[r].data() + p.err_off, 0, p.nseg * p.seg_bytes);
        for (size_t j = 0; j < p.nseg; ++j)
            HostQuantize(in.data() + j * p.seg_bytes, buf[r].data() + p.err_off + j * p.seg_bytes,
                         buf[r].data() + j * p.seg_wire, p.count, p.block, dt, true);
    }
    // the exchange by hand: each send lands where the receiver's step of the
    // same phase points
    for (int r = 0; r < N; ++r)
        for (const Step& st : sch[r].steps)
            for (const Step& pt : sch[st.send_peer].steps)
                if (pt.phase == st.phase && pt.recv_peer == r)
                    std::memcpy(buf[st.send_peer].data() + plan[st.send_peer].scratch_off +
                                    pt.recv.off,
                                buf[r].data() + st.send.off, st.send.bytes);
    for (int r = 0; r < N; ++r) {
        // the plan's wire table: ascending rank order, own segment at r
        const void* wires[8];
        for (int k = 0; k < plan[r].nwires; ++k) wires[k] = buf[r].data() + plan[r].wire_off[k];
        std::vector<uint8_t> out(count * es, 0xCD), want(count * es);
        HostQuantSumDequantN(wires, plan[r].nwires, out.data(), count, block, dt);
        for (size_t i = 0; i < count; ++i) {
            float acc = 0.f;
            for (int p = 0; p < N; ++p) {
                // rank p's wire of segment r, straight from where p quantized it
                const uint8_t* wb = buf[p].data() + r * segB + (i / block) * (block + 8);
                float scale;
                std::memcpy(&scale, wb, 4);
                acc = std::fmaf(static_cast<float>(static_cast<int8_t>(wb[8 + i % block])),
                                scale, acc);
            }
            if (dt == DataType::F32) std::memcpy(&want[i * 4], &acc, 4);
            else {
                const uint16_t h = ToBf16(acc);
                std::memcpy(&want[i * 2], &h, 2);
            }
        }
        EXPECT(std::memcmp(out.data(), want.data(), out.size()) == 0,
               "exchange N=%d r=%d count=%zu block=%zu es=%zu: result differs", N, r, count,
               block, es);
    }
}

static void TestRejects() {
    std::vector<uint8_t> w(264, 0), out(1024, 0);
    const void* wires[9];
    for (auto& p : wires) p = w.data();
    auto throws = [&](int n, DataType dt) {
        try {
            HostQuantSumDequantN(wires, n, out.data(), 4, 256, dt);
        } catch (const std::exception&) {
            return true;
        }
        return false;
    };
    EXPECT(throws(0, DataType::F32), "0 wires accepted");
    EXPECT(throws(9, DataType::F32), "9 wires accepted");
    EXPECT(throws(2, DataType::F64), "f64 accepted");
    EXPECT(!throws(8, DataType::F32), "8 wires rejected");
}

int main() {
    for (int N = 1; N <= 9; ++N) {
        TestSchedule(N, 1, 256);
        TestSchedule(N, 5, 128);
    }
    for (Algo algo : {Algo::ALLREDUCE, Algo::RING, Algo::DIRECT})
        for (int N = 1; N <= 9; ++N)
            for (size_t es : {2, 4}) {
                TestPlan(algo, N, 1, 256, es);
                TestPlan(algo, N, 5, 128, es);
                // 3 x 5 x 264 = 3960 is no multiple of 16: padding behind the wire
                // at world 3, and behind a one-slot scratch at world 2
                TestPlan(algo, N, 5, 256, es);
            }
    for (int N = 2; N <= 8; ++N)
        for (DataType dt : {DataType::F32, DataType::BF16}) {
            TestExchange(N, 1003, 128, dt);
            TestExchange(N, 1280, 256, dt);
        }
    TestRejects();
    if (g_failures) {
        std::printf("%d FAILURES\n", g_failures);
        return 1;
    }
    std::printf("quant_rs_direct_selftest: PASS\n");
    return 0;
}
