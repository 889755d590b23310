// Pure-host test of the one-shot (direct) quantized reduce-scatter, built
// with ASan/UBSan and run by pytest (tests/test_quant_rs_direct_cpu.py):
//   - BuildReduceScatterDirectUnits for worlds 1..9: the simulator accepts
//     the schedules (every send has a matching receive of the same size),
//     the receive slots are disjoint and cover tmp_bytes, and wire segment
//     `to` goes to rank `to` and lands in the slot the epilogue reads;
//   - HostQuantize -> the exchange walked by hand -> HostQuantSumDequantN
//     for worlds 2..8 against the sum of the dequantized wires in rank order
//     with one fmaf per wire.
// Exit 0 = PASS.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../comm/quant.hpp"
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

// slot of peer `from` in rank r's TMP: ascending rank order, r left out
static size_t SlotOf(int from, int r) { return static_cast<size_t>(from < r ? from : from - 1); }

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
                       st.recv.off == SlotOf(st.recv_peer, r) * segB,
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
    // inputs: a different magnitude per rank, so the block scales differ
    std::vector<std::vector<uint8_t>> wire(N), tmp(N);
    uint32_t lcg = 12345u + static_cast<uint32_t>(N);
    for (int r = 0; r < N; ++r) {
        std::vector<uint8_t> in(N * count * es), err(N * count * es, 0);
        for (size_t i = 0; i < N * count; ++i) {
            lcg = lcg * 1664525u + 1013904223u;
            const float v = (static_cast<float>(lcg >> 8) / 8388608.f - 1.f) * (1.f + r);
            if (dt == DataType::F32) std::memcpy(&in[i * 4], &v, 4);
            else {
                const uint16_t h = ToBf16(v);
                std::memcpy(&in[i * 2], &h, 2);
            }
        }
        wire[r].assign(N * segB, 0);
        tmp[r].assign(sch[r].tmp_bytes, 0xAB);
        for (int j = 0; j < N; ++j)
            HostQuantize(in.data() + j * count * es, err.data() + j * count * es,
                         wire[r].data() + j * segB, count, block, dt, true);
    }
    // the exchange by hand: each send lands where the receiver's step of the
    // same phase points
    for (int r = 0; r < N; ++r)
        for (const Step& st : sch[r].steps)
            for (const Step& pt : sch[st.send_peer].steps)
                if (pt.phase == st.phase && pt.recv_peer == r)
                    std::memcpy(tmp[st.send_peer].data() + pt.recv.off,
                                wire[r].data() + st.send.off, st.send.bytes);
    for (int r = 0; r < N; ++r) {
        // pointer table in ascending rank order, own segment at position r
        const void* wires[8];
        for (int p = 0; p < N; ++p)
            wires[p] = p == r ? wire[r].data() + r * segB
                              : tmp[r].data() + sch[r].result.off + SlotOf(p, r) * segB;
        std::vector<uint8_t> out(count * es, 0xCD), want(count * es);
        HostQuantSumDequantN(wires, N, out.data(), count, block, dt);
        for (size_t i = 0; i < count; ++i) {
            float acc = 0.f;
            for (int p = 0; p < N; ++p) {
                // rank p's wire of segment r, straight from where p quantized it
                const uint8_t* wb = wire[p].data() + r * segB + (i / block) * (block + 8);
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
