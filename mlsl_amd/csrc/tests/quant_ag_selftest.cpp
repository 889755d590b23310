// Pure-host test of the quantized all-gather, built with ASan/UBSan and run by
// pytest (tests/test_quant_ag_cpu.py):
//   - BuildAllGatherUnits for worlds 1..9: the simulator accepts the
//     schedules, every rank receives every other rank's segment exactly once
//     and into that segment's own place, every send reads segment `rank`
//     only, there are no local ops and no TMP, and `result` is the whole wire;
//   - MakeQuantPlan for those schedules, every rank, both finish modes:
//     one send segment quantized into wire segment `me`, N output segments,
//     no residual region, padded regions that `bytes` covers;
//   - HostQuantize (no residual) -> the exchange walked by hand inside one
//     plan-sized buffer per rank -> HostDequantizeSegments, for worlds 1..9,
//     against the segments decoded one element at a time, assigned and
//     accumulated; recv is the same on every rank;
//   - HostDequantizeSegments rejects f64, no segments and a block of 6.
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
    for (int r = 0; r < N; ++r) sch[r] = BuildAllGatherUnits(r, N, units, block + 8, block);
    return sch;
}

static void TestSchedule(int N, size_t units, size_t block) {
    const size_t segB = units * (block + 8);
    std::vector<Schedule> sch = Build(N, units, block);
    for (int r = 0; r < N; ++r) {
        const Schedule& s = sch[r];
        EXPECT(s.dtype == DataType::U8 && s.quant_block == block, "N=%d r=%d header", N, r);
        EXPECT(s.wire_bytes == N * segB, "N=%d r=%d wire_bytes %zu", N, r, s.wire_bytes);
        EXPECT(s.tmp_bytes == 0 && s.fan_in == 0 && !s.one_shot, "N=%d r=%d scratch", N, r);
        EXPECT(s.result.space != Space::TMP && s.result.off == 0 &&
                   s.result.bytes == s.wire_bytes, "N=%d r=%d result", N, r);
        EXPECT(s.steps.size() == static_cast<size_t>(N - 1) && s.num_phases == N - 1,
               "N=%d r=%d: %zu steps, %d phases", N, r, s.steps.size(), s.num_phases);
        std::vector<int> sent_to(N, 0), got_from(N, 0);
        for (const Step& st : s.steps) {
            EXPECT(st.local == Step::LocalOp::NONE, "N=%d r=%d: local op", N, r);
            EXPECT(st.send_peer >= 0 && st.send_peer < N && st.send_peer != r &&
                       st.recv_peer >= 0 && st.recv_peer < N && st.recv_peer != r,
                   "N=%d r=%d peers %d %d", N, r, st.send_peer, st.recv_peer);
            if (st.send_peer < 0 || st.send_peer >= N || st.recv_peer < 0 || st.recv_peer >= N)
                return;
            // exchange j is phase j-1, with (rank+j)%N and (rank-j+N)%N
            const int j = st.phase + 1;
            EXPECT(st.send_peer == (r + j) % N && st.recv_peer == (r - j + N) % N,
                   "N=%d r=%d phase %d: peers %d %d", N, r, st.phase, st.send_peer,
                   st.recv_peer);
            // sends read this rank's segment only
            EXPECT(st.send.space != Space::TMP && st.send.bytes == segB &&
                       st.send.off == static_cast<size_t>(r) * segB,
                   "N=%d r=%d: send reads off %zu", N, r, st.send.off);
            // segment `from` lands in its own place in the wire
            EXPECT(st.recv.space != Space::TMP && st.recv.bytes == segB &&
                       st.recv.off == static_cast<size_t>(st.recv_peer) * segB,
                   "N=%d r=%d: recv from %d lands at %zu", N, r, st.recv_peer, st.recv.off);
            ++sent_to[st.send_peer];
            ++got_from[st.recv_peer];
        }
        for (int p = 0; p < N; ++p)
            EXPECT(sent_to[p] == (p != r) && got_from[p] == (p != r),
                   "N=%d r=%d peer %d: %d sends %d recvs", N, r, p, sent_to[p], got_from[p]);
    }
    // The simulator keeps SEND and RECV apart: give every rank its own
    // segment in both, and afterwards RECV must hold every rank's segment.
    std::vector<std::vector<uint8_t>> sbuf(N), rbuf(N);
    for (int r = 0; r < N; ++r) {
        sbuf[r].assign(N * segB, 0);
        rbuf[r].assign(N * segB, 0);
        std::memset(sbuf[r].data() + r * segB, r + 1, segB);
        std::memset(rbuf[r].data() + r * segB, r + 1, segB);
    }
    try {
        SimulateSchedules(sch, sbuf, rbuf);
    } catch (const std::exception& e) {
        EXPECT(false, "N=%d simulator: %s", N, e.what());
        return;
    }
    for (int r = 0; r < N; ++r)
        for (int p = 0; p < N; ++p) {
            bool ok = true;
            for (size_t i = 0; i < segB; ++i) ok = ok && rbuf[r][p * segB + i] == p + 1;
            EXPECT(ok, "N=%d r=%d: segment %d did not arrive", N, r, p);
        }
}

static size_t Al16(size_t x) { return (x + 15) / 16 * 16; }

static void TestPlan(int N, size_t units, size_t block, size_t es, bool accumulate) {
    const size_t segB = units * (block + 8);
    const size_t count = units * block - 3;
    for (int r = 0; r < N; ++r) {
        const Schedule sch = BuildAllGatherUnits(r, N, units, block + 8, block);
        const QuantPlan p = MakeQuantPlan(
            sch, N, r, count, es, accumulate ? QuantGather::ACCUMULATE : QuantGather::ASSIGN);
        EXPECT(p.block == block && p.count == count && p.seg_bytes == count * es &&
                   p.seg_wire == segB, "plan N=%d r=%d: strides", N, r);
        EXPECT(p.nseg == 1 && p.send_seg == static_cast<size_t>(r) && !p.residual,
               "plan N=%d r=%d: nseg %zu send_seg %zu residual %d", N, r, p.nseg, p.send_seg,
               p.residual);
        EXPECT(p.finish == QuantFinish::SCATTER && p.out_segs == static_cast<size_t>(N) &&
                   p.accumulate == accumulate && p.nwires == 1 && p.wire_off[0] == 0,
               "plan N=%d r=%d: finish", N, r);
        // wire, then (empty) scratch, then an empty residual region
        const size_t wire_end = N * segB;
        EXPECT(p.scratch_off == Al16(wire_end) && p.err_off == p.scratch_off &&
                   p.bytes == p.err_off,
               "plan N=%d r=%d: offsets %zu %zu %zu", N, r, p.scratch_off, p.err_off, p.bytes);
        EXPECT(p.scratch_off % 16 == 0 && p.err_off % 16 == 0 && p.bytes % 16 == 0 &&
                   wire_end <= p.bytes && (p.send_seg + p.nseg) * p.seg_wire <= wire_end,
               "plan N=%d r=%d: regions", N, r);
    }
    // the shapes the plan must keep refusing
    bool threw = false;
    try {
        MakeQuantPlan(BuildReduceScatterUnits(0, 3, units, block + 8, block), 3, 0, count, es,
                      QuantGather::ASSIGN);
    } catch (const std::exception&) {
        threw = true;
    }
    EXPECT(threw, "a reduce-scatter schedule passed for an all-gather");
}

static float FromBf16(uint16_t h) {
    const uint32_t u = static_cast<uint32_t>(h) << 16;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

static uint16_t ToBf16(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1);
    return static_cast<uint16_t>(u >> 16);
}

static void PutElem(std::vector<uint8_t>& buf, size_t i, float v, DataType dt) {
    if (dt == DataType::F32) std::memcpy(&buf[i * 4], &v, 4);
    else {
        const uint16_t h = ToBf16(v);
        std::memcpy(&buf[i * 2], &h, 2);
    }
}

static float GetElem(const std::vector<uint8_t>& buf, size_t i, DataType dt) {
    if (dt == DataType::F32) {
        float v;
        std::memcpy(&v, &buf[i * 4], 4);
        return v;
    }
    uint16_t h;
    std::memcpy(&h, &buf[i * 2], 2);
    return FromBf16(h);
}

static void TestExchange(int N, size_t count, size_t block, DataType dt, bool accumulate) {
    const size_t es = dt == DataType::F32 ? 4 : 2;
    const size_t units = (count + block - 1) / block;
    const size_t segB = units * (block + 8);
    std::vector<Schedule> sch = Build(N, units, block);
    std::vector<QuantPlan> plan(N);
    std::vector<std::vector<uint8_t>> buf(N);
    uint32_t lcg = 4321u + static_cast<uint32_t>(N);
    auto next = [&]() {
        lcg = lcg * 1664525u + 1013904223u;
        return static_cast<float>(lcg >> 8) / 8388608.f - 1.f;
    };
    for (int r = 0; r < N; ++r) {
        std::vector<uint8_t> in(count * es);
        for (size_t i = 0; i < count; ++i) PutElem(in, i, next() * (1.f + r), dt);
        const QuantPlan& p = plan[r] = MakeQuantPlan(
            sch[r], N, r, count, es, accumulate ? QuantGather::ACCUMULATE : QuantGather::ASSIGN);
        // exactly plan-sized: ASan sees any access past the plan's regions
        buf[r].assign(p.bytes, 0xAB);
        for (size_t j = 0; j < p.nseg; ++j)
            HostQuantize(in.data() + j * p.seg_bytes, nullptr,
                         buf[r].data() + (p.send_seg + j) * p.seg_wire, p.count, p.block, dt,
                         p.residual);
    }
    // the exchange by hand: SEND and RECV refs both address the wire
    for (int r = 0; r < N; ++r)
        for (const Step& st : sch[r].steps)
            for (const Step& pt : sch[st.send_peer].steps)
                if (pt.phase == st.phase && pt.recv_peer == r)
                    std::memcpy(buf[st.send_peer].data() + pt.recv.off,
                                buf[r].data() + st.send.off, st.send.bytes);
    // recv on entry: the same on every rank, as the accumulate mode needs
    std::vector<uint8_t> recv0(N * count * es);
    for (size_t i = 0; i < N * count; ++i) PutElem(recv0, i, next() * 4.f, dt);
    std::vector<uint8_t> want(N * count * es);
    for (int p = 0; p < N; ++p)
        for (size_t i = 0; i < count; ++i) {
            // rank p's wire, straight from where p quantized it
            const uint8_t* wb = buf[p].data() + p * segB + (i / block) * (block + 8);
            float scale;
            std::memcpy(&scale, wb, 4);
            const float q = static_cast<float>(static_cast<int8_t>(wb[8 + i % block]));
            const float v = accumulate ? std::fmaf(q, scale, GetElem(recv0, p * count + i, dt))
                                       : q * scale;
            PutElem(want, p * count + i, v, dt);
        }
    for (int r = 0; r < N; ++r) {
        std::vector<uint8_t> out = recv0;
        HostDequantizeSegments(buf[r].data() + plan[r].wire_off[0], plan[r].out_segs, out.data(),
                               count, block, dt, plan[r].accumulate);
        EXPECT(std::memcmp(out.data(), want.data(), out.size()) == 0,
               "exchange N=%d r=%d count=%zu block=%zu es=%zu acc=%d: result differs", N, r,
               count, block, es, accumulate);
    }
}

static void TestRejects() {
    std::vector<uint8_t> w(264, 0), out(1024, 0x5A);
    auto throws = [&](size_t nseg, size_t block, DataType dt) {
        try {
            HostDequantizeSegments(w.data(), nseg, out.data(), 4, block, dt, false);
        } catch (const std::exception&) {
            return true;
        }
        return false;
    };
    EXPECT(throws(0, 256, DataType::F32), "0 segments accepted");
    EXPECT(throws(1, 6, DataType::F32), "block 6 accepted");
    EXPECT(throws(1, 256, DataType::F64), "f64 accepted");
    bool untouched = true;
    for (uint8_t b : out) untouched = untouched && b == 0x5A;
    EXPECT(untouched, "a rejected call wrote to out");
    EXPECT(!throws(1, 256, DataType::F32), "a legal call was rejected");
}

int main() {
    for (int N = 1; N <= 9; ++N) {
        TestSchedule(N, 1, 256);
        TestSchedule(N, 5, 128);
        for (size_t es : {2, 4})
            for (bool acc : {false, true}) {
                TestPlan(N, 1, 256, es, acc);
                TestPlan(N, 5, 128, es, acc);
                // 3 x 5 x 264 = 3960 is no multiple of 16: padding behind the wire
                TestPlan(N, 5, 256, es, acc);
            }
        for (DataType dt : {DataType::F32, DataType::BF16})
            for (bool acc : {false, true}) {
                TestExchange(N, 1003, 128, dt, acc);
                TestExchange(N, 1280, 256, dt, acc);
            }
    }
    TestRejects();
    if (g_failures) {
        std::printf("%d FAILURES\n", g_failures);
        return 1;
    }
    std::printf("quant_ag_selftest: PASS\n");
    return 0;
}
