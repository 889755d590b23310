// Pure-host test of the two-shot quantized allreduce, built with ASan/UBSan
// and run by pytest (tests/test_quant_ar_cpu.py):
//   - BuildAllReduceTwoShotUnits for worlds 1..9 at 1, 5, 8 and 17 units (some
//     ranks own nothing): phase-A slots are disjoint and cover tmp_bytes,
//     range `to` goes to rank `to`, phase B puts every range in its place, the
//     one SUMQ step is the only local op, every send has a matching receive
//     of the same size, and the simulator refuses the schedule by name;
//   - MakeQuantPlan's SUMQ table for every rank against formulas written out
//     here, and its absence from the plans of the other unit schedules;
//   - HostQuantize -> phase A walked by hand -> HostQuantSumRequantN -> phase B
//     walked by hand -> HostDequantize for worlds 1..8, all inside one buffer
//     of exactly plan.bytes per rank: equal on all ranks and equal to a direct
//     computation written out here.
// Exit 0 = PASS.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
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

static std::vector<Schedule> Build(int N, size_t units, size_t block) {
    std::vector<Schedule> sch(N);
    for (int r = 0; r < N; ++r)
        sch[r] = BuildAllReduceTwoShotUnits(r, N, units, block + 8, block);
    return sch;
}

// ownership written out: rank i owns units [i*units/N, (i+1)*units/N)
static size_t Lo(size_t units, int N, int i) { return static_cast<size_t>(i) * units / N; }
static size_t Cnt(size_t units, int N, int i) { return Lo(units, N, i + 1) - Lo(units, N, i); }

static bool SameRef(const BufRef& b, Space sp, size_t off, size_t bytes) {
    return b.space == sp && b.off == off && b.bytes == bytes;
}

static void TestSchedule(int N, size_t units, size_t block) {
    const size_t U = block + 8;
    std::vector<Schedule> sch = Build(N, units, block);
    for (int r = 0; r < N; ++r) {
        const Schedule& s = sch[r];
        const size_t own_off = Lo(units, N, r) * U, own_b = Cnt(units, N, r) * U;
        EXPECT(s.dtype == DataType::U8 && s.quant_block == block && s.fan_in == 0 &&
                   !s.one_shot, "N=%d r=%d header", N, r);
        EXPECT(s.wire_bytes == units * U, "N=%d r=%d wire_bytes %zu", N, r, s.wire_bytes);
        EXPECT(SameRef(s.result, Space::SEND, 0, units * U), "N=%d r=%d result", N, r);
        if (N == 1) {
            EXPECT(s.steps.empty() && s.num_phases == 0 && s.tmp_bytes == 0,
                   "N=1 must have no steps and no TMP");
            continue;
        }
        EXPECT(s.steps.size() == static_cast<size_t>(2 * N - 1) && s.num_phases == 2 * N - 1,
               "N=%d r=%d: %zu steps, %d phases", N, r, s.steps.size(), s.num_phases);
        EXPECT(s.tmp_bytes == (N - 1) * own_b, "N=%d r=%d tmp_bytes %zu", N, r, s.tmp_bytes);
        std::vector<size_t> slots;
        std::vector<int> a_to(N, 0), a_from(N, 0), b_to(N, 0), b_from(N, 0);
        int local_ops = 0, last_phase = -1;
        for (const Step& st : s.steps) {
            EXPECT(st.phase >= last_phase, "N=%d r=%d: steps not sorted by phase", N, r);
            last_phase = st.phase;
            if (st.phase == N - 1) {
                ++local_ops;
                EXPECT(st.local == Step::LocalOp::SUMQ && st.send_peer < 0 && st.recv_peer < 0,
                       "N=%d r=%d: phase N-1 is the requantize alone", N, r);
                EXPECT(SameRef(st.local_src, Space::TMP, 0, s.tmp_bytes) &&
                           SameRef(st.local_dst, Space::SEND, own_off, own_b),
                       "N=%d r=%d: SUMQ ranges", N, r);
                continue;
            }
            EXPECT(st.local == Step::LocalOp::NONE, "N=%d r=%d phase %d: local op", N, r,
                   st.phase);
            const int to = st.send_peer, from = st.recv_peer;
            EXPECT(to >= 0 && to < N && to != r && from >= 0 && from < N && from != r,
                   "N=%d r=%d peers %d %d", N, r, to, from);
            if (to < 0 || to >= N || from < 0 || from >= N) return;
            if (st.phase < N - 1) {
                // range `to` goes to rank `to`; arrivals in ascending rank order
                EXPECT(SameRef(st.send, Space::SEND, Lo(units, N, to) * U, Cnt(units, N, to) * U),
                       "N=%d r=%d: send to %d reads off %zu", N, r, to, st.send.off);
                EXPECT(SameRef(st.recv, Space::TMP, (from - (from > r)) * own_b, own_b),
                       "N=%d r=%d: recv from %d lands at %zu", N, r, from, st.recv.off);
                ++a_to[to];
                ++a_from[from];
                slots.push_back(st.recv.off);
            } else {
                // the own range goes out; from's range lands in its place
                EXPECT(SameRef(st.send, Space::SEND, own_off, own_b),
                       "N=%d r=%d: gather send off %zu", N, r, st.send.off);
                EXPECT(st.recv.space != Space::TMP && st.recv.off == Lo(units, N, from) * U &&
                           st.recv.bytes == Cnt(units, N, from) * U,
                       "N=%d r=%d: gather recv from %d at %zu", N, r, from, st.recv.off);
                ++b_to[to];
                ++b_from[from];
            }
            // the receiver expects this rank in the same phase, with this size
            bool matched = false;
            for (const Step& pt : sch[to].steps)
                matched = matched || (pt.phase == st.phase && pt.recv_peer == r &&
                                      pt.recv.bytes == st.send.bytes);
            EXPECT(matched, "N=%d r=%d phase %d: rank %d does not receive", N, r, st.phase, to);
        }
        EXPECT(local_ops == 1, "N=%d r=%d: %d local ops", N, r, local_ops);
        for (int p = 0; p < N; ++p)
            EXPECT(a_to[p] == (p != r) && a_from[p] == (p != r) && b_to[p] == (p != r) &&
                       b_from[p] == (p != r), "N=%d r=%d peer %d: exchange counts", N, r, p);
        std::sort(slots.begin(), slots.end());
        for (size_t k = 0; k < slots.size(); ++k)
            EXPECT(slots[k] == k * own_b, "N=%d r=%d slot %zu at %zu", N, r, k, slots[k]);
    }
    // SUMQ is not a REDUCE: the simulator refuses the schedule, and says why
    std::vector<std::vector<uint8_t>> sbuf(N), rbuf(N);
    for (int r = 0; r < N; ++r) {
        sbuf[r].assign(units * U, static_cast<uint8_t>(r + 1));
        rbuf[r] = sbuf[r];
    }
    std::string what;
    try {
        SimulateSchedules(sch, sbuf, rbuf);
    } catch (const std::exception& e) {
        what = e.what();
    }
    EXPECT((N == 1) == what.empty() && (N == 1 || what.find("SUMQ") != std::string::npos),
           "N=%d simulator: '%s'", N, what.c_str());
    for (int r = 0; r < N; ++r)
        EXPECT(sbuf[r] == std::vector<uint8_t>(units * U, static_cast<uint8_t>(r + 1)),
               "N=%d r=%d: the refused simulation wrote a buffer", N, r);
}

static size_t Al16(size_t x) { return (x + 15) / 16 * 16; }

static void TestPlan(int N, size_t units, size_t block, size_t es) {
    const size_t U = block + 8;
    const size_t count = units * block - 3;   // a tail block
    for (int r = 0; r < N; ++r) {
        const Schedule sch = BuildAllReduceTwoShotUnits(r, N, units, U, block);
        QuantPlan p;
        bool threw = false;
        try {
            p = MakeQuantPlan(sch, 1, r, count, es);
        } catch (const std::exception&) {
            threw = true;
        }
        EXPECT(threw == (N > 8), "plan N=%d r=%d: threw=%d", N, r, threw);
        if (threw) continue;
        const size_t own_off = Lo(units, N, r) * U, own_b = Cnt(units, N, r) * U;
        const size_t tmp = N == 1 ? 0 : (N - 1) * own_b;
        const size_t scratch = Al16(units * U), err = scratch + Al16(tmp);
        // prologue and finish are the flat allreduce's
        EXPECT(p.block == block && p.count == count && p.nseg == 1 && p.send_seg == 0 &&
                   p.residual && p.seg_bytes == count * es && p.seg_wire == units * U,
               "plan N=%d r=%d: prologue", N, r);
        EXPECT(p.scratch_off == scratch && p.err_off == err &&
                   p.bytes == err + Al16(count * es) && sch.tmp_bytes == tmp,
               "plan N=%d r=%d: offsets %zu %zu %zu", N, r, p.scratch_off, p.err_off, p.bytes);
        EXPECT(p.finish == QuantFinish::DEQUANT && p.nwires == 1 && p.wire_off[0] == 0,
               "plan N=%d r=%d: finish", N, r);
        if (N == 1) {
            EXPECT(p.sumq_nwires == 0 && p.sumq_units == 0, "plan N=1: SUMQ table");
            continue;
        }
        EXPECT(p.sumq_nwires == N && p.sumq_dst_off == own_off &&
                   p.sumq_units == Cnt(units, N, r),
               "plan N=%d r=%d: SUMQ %d wires, dst %zu, %zu units", N, r, p.sumq_nwires,
               p.sumq_dst_off, p.sumq_units);
        for (int q = 0; q < N && q < 8; ++q) {
            const size_t want = q == r ? own_off : scratch + (q - (q > r)) * own_b;
            EXPECT(p.sumq_wire_off[q] == want, "plan N=%d r=%d: SUMQ wire %d at %zu", N, r, q,
                   p.sumq_wire_off[q]);
            // a whole wire inside the wire region or inside the scratch
            const size_t lo = p.sumq_wire_off[q], hi = lo + own_b;
            EXPECT(hi <= units * U || (lo >= scratch && hi <= scratch + tmp),
                   "plan N=%d r=%d: SUMQ wire %d outside its region", N, r, q);
        }
    }
    // no other unit schedule grows a SUMQ table
    for (int r = 0; r < N; ++r) {
        const size_t me = static_cast<size_t>(r), n = static_cast<size_t>(N);
        std::vector<QuantPlan> plans = {
            MakeQuantPlan(BuildAllReduceRingUnits(r, N, units, U, block), 1, me, count, es),
            MakeQuantPlan(BuildReduceScatterUnits(r, N, units, U, block), n, me, count, es),
            MakeQuantPlan(BuildAllGatherUnits(r, N, units, U, block), n, me, count, es,
                          QuantGather::ASSIGN)};
        if (N <= 8)   // the one-shot reduce-scatter's own limit
            plans.push_back(MakeQuantPlan(BuildReduceScatterDirectUnits(r, N, units, U, block),
                                          n, me, count, es));
        for (const QuantPlan& p : plans)
            EXPECT(p.sumq_nwires == 0 && p.sumq_units == 0 && p.sumq_dst_off == 0,
                   "plan N=%d r=%d: SUMQ table without a SUMQ step", N, r);
    }
}

static uint16_t ToBf16(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1);
    return static_cast<uint16_t>(u >> 16);
}

// where a BufRef of rank r's schedule lives inside its plan-sized buffer
static uint8_t* At(std::vector<uint8_t>& buf, const QuantPlan& p, const BufRef& b) {
    return buf.data() + (b.space == Space::TMP ? p.scratch_off : 0) + b.off;
}

static void TestExchange(int N, size_t count, size_t block, DataType dt) {
    const size_t es = dt == DataType::F32 ? 4 : 2;
    const size_t units = (count + block - 1) / block, U = block + 8;
    std::vector<Schedule> sch = Build(N, units, block);
    std::vector<QuantPlan> plan(N);
    std::vector<std::vector<uint8_t>> buf(N), first(N);
    uint32_t lcg = 777u + static_cast<uint32_t>(N);
    for (int r = 0; r < N; ++r) {
        std::vector<uint8_t> in(count * es);
        for (size_t i = 0; i < count; ++i) {
            lcg = lcg * 1664525u + 1013904223u;
            const float v = (static_cast<float>(lcg >> 8) / 8388608.f - 1.f) * (1.f + r);
            if (dt == DataType::F32) std::memcpy(&in[i * 4], &v, 4);
            else {
                const uint16_t h = ToBf16(v);
                std::memcpy(&in[i * 2], &h, 2);
            }
        }
        const QuantPlan& p = plan[r] = MakeQuantPlan(sch[r], 1, r, count, es);
        buf[r].assign(p.bytes, 0xAB);   // exactly plan.bytes: ASan guards the rest
        std::memset(buf[r].data() + p.err_off, 0, p.seg_bytes);
        HostQuantize(in.data(), buf[r].data() + p.err_off, buf[r].data(), p.count, p.block, dt,
                     true);
        first[r].assign(buf[r].begin(), buf[r].begin() + units * U);
    }
    // each send of phases [lo, hi) lands where the receiver's step of the
    // same phase points
    auto exchange = [&](int lo, int hi) {
        for (int phase = lo; phase < hi; ++phase)
            for (int r = 0; r < N; ++r)
                for (const Step& st : sch[r].steps) {
                    if (st.phase != phase || st.send_peer < 0 || st.send.bytes == 0) continue;
                    const int to = st.send_peer;
                    for (const Step& pt : sch[to].steps)
                        if (pt.phase == phase && pt.recv_peer == r)
                            std::memcpy(At(buf[to], plan[to], pt.recv),
                                        At(buf[r], plan[r], st.send), st.send.bytes);
                }
    };
    exchange(0, N - 1);
    for (int r = 0; r < N && N > 1; ++r) {
        const QuantPlan& p = plan[r];
        const void* wires[8];
        for (int k = 0; k < p.sumq_nwires; ++k) wires[k] = buf[r].data() + p.sumq_wire_off[k];
        if (p.sumq_units)
            HostQuantSumRequantN(wires, p.sumq_nwires, buf[r].data() + p.sumq_dst_off,
                                 p.sumq_units, p.block);
    }
    exchange(N, 2 * N - 1);
    // the direct computation: unit by unit from the first quantization
    std::vector<uint8_t> want(count * es);
    for (size_t u = 0; u < units; ++u) {
        std::vector<float> acc(block, 0.f);
        float m = 0.f;
        for (size_t i = 0; i < block; ++i) {
            for (int p = 0; p < N && N > 1; ++p) {
                const uint8_t* wb = first[p].data() + u * U;
                float scale;
                std::memcpy(&scale, wb, 4);
                acc[i] = std::fmaf(static_cast<float>(static_cast<int8_t>(wb[8 + i])), scale,
                                   acc[i]);
            }
            m = std::max(m, std::fabs(acc[i]));
        }
        float scale = m > 0.f ? m / 127.f : 1.f;
        const float inv = 1.f / scale;
        for (size_t i = 0; i < block && u * block + i < count; ++i) {
            // through int8, as on the wire: a -0 becomes +0
            float q = static_cast<float>(static_cast<int8_t>(
                std::min(127.f, std::max(-127.f, std::nearbyint(acc[i] * inv)))));
            if (N == 1) {   // nothing is requantized on a group of one
                const uint8_t* wb = first[0].data() + u * U;
                std::memcpy(&scale, wb, 4);
                q = static_cast<float>(static_cast<int8_t>(wb[8 + i]));
            }
            const float v = q * scale;
            const size_t e = u * block + i;
            if (dt == DataType::F32) std::memcpy(&want[e * 4], &v, 4);
            else {
                const uint16_t h = ToBf16(v);
                std::memcpy(&want[e * 2], &h, 2);
            }
        }
    }
    for (int r = 0; r < N; ++r) {
        const QuantPlan& p = plan[r];
        std::vector<uint8_t> out(count * es, 0xCD);
        HostDequantize(buf[r].data() + p.wire_off[0], out.data(), count, block, dt);
        EXPECT(out == want, "exchange N=%d r=%d count=%zu block=%zu es=%zu: result differs", N,
               r, count, block, es);
        // the whole wire, headers included, is the same on all ranks
        EXPECT(std::memcmp(buf[r].data(), buf[0].data(), units * U) == 0,
               "exchange N=%d r=%d: wire differs from rank 0's", N, r);
    }
}

static void TestRejects() {
    std::vector<uint8_t> w(264, 0), dst(264, 0xAB);
    const void* wires[9];
    for (auto& p : wires) p = w.data();
    auto throws = [&](int n, size_t block) {
        try {
            HostQuantSumRequantN(wires, n, dst.data(), 1, block);
        } catch (const std::exception&) {
            return true;
        }
        return false;
    };
    EXPECT(throws(0, 256), "0 wires accepted");
    EXPECT(throws(9, 256), "9 wires accepted");
    EXPECT(throws(2, 0), "block 0 accepted");
    EXPECT(throws(2, 6), "block 6 accepted");
    EXPECT(dst == std::vector<uint8_t>(264, 0xAB), "a rejected call wrote");
    EXPECT(!throws(8, 256), "8 wires rejected");
    // all-zero wires: scale 1, second header word 0, payload 0
    float hdr[2];
    std::memcpy(hdr, dst.data(), 8);
    EXPECT(hdr[0] == 1.f && hdr[1] == 0.f &&
               std::all_of(dst.begin() + 8, dst.end(), [](uint8_t b) { return b == 0; }),
           "zero block");
}

int main() {
    for (int N = 1; N <= 9; ++N)
        for (size_t units : {1, 5, 8, 17}) {
            TestSchedule(N, units, units == 5 ? 128 : 256);
            for (size_t es : {2, 4}) TestPlan(N, units, units == 5 ? 128 : 256, es);
        }
    for (int N = 1; N <= 8; ++N)
        for (DataType dt : {DataType::F32, DataType::BF16}) {
            TestExchange(N, 1003, 128, dt);   // 8 units, a tail block
            TestExchange(N, 1280, 256, dt);   // 5 units: ranks that own nothing from N = 6
            TestExchange(N, 200, 256, dt);    // 1 unit: one owner
        }
    TestRejects();
    if (g_failures) {
        std::printf("%d FAILURES\n", g_failures);
        return 1;
    }
    std::printf("quant_ar_twoshot_selftest: PASS\n");
    return 0;
}
