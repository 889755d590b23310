// Host-only launch trace of the IPC-window schedule walker
// (P2pGroup::IssueSchedule), built with g++ and ASan/UBSan and run by pytest
// (tests/test_p2p_issue_trace.py). No device is touched: the group is put
// together by hand over fake addresses that nothing dereferences, and the
// recording launchers of asan_kernel_stubs.cpp write one line per launch.
//
// Every case runs for every rank of its group on a fresh group object: the
// schedule is issued twice on lane 0 and once on lane 1, so sequence numbers,
// slot wrap, ack targets and the absolute counter targets carry across calls.
// Schedules and plans come from the real builders. One line per (case, rank)
// goes to stdout: the number of launches and the FNV-1a digest of the trace
// text; tests/golden/p2p_issue_trace.txt holds these lines for
// MLSL_P2P_FUSED_MAX_KB unset and for 0 (the walker reads it once per
// process, so the matrix runs once per setting). `--dump CASE` prints the
// text itself.
//
// "small" fits one fused sub-message; "large" is 3 MiB per transferred
// segment against 1 MiB slots, two per edge: backpressure waits appear and
// the slot index wraps. The local op that both device walkers share is traced
// directly as well, once per op kind with nontemporal copies, which is how
// the RCCL walker calls it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../comm/device_local_op.hpp"
#include "../comm/p2p_transport.hpp"
#include "../comm/quant_plan.hpp"
#include "../comm/request.hpp"
#include "../comm/schedule.hpp"

namespace mlsl {

extern std::string* g_kernel_trace;

namespace {
template <class T>
T* Fake(uint64_t k, uint64_t off = 0) {
    return reinterpret_cast<T*>((k << 40) + off);
}
constexpr size_t kLanes = 2, kSlots = 2, kSlotBytes = 1u << 20;

}  // namespace

// Builds a P2pGroup without Create(): no window, no IPC, no bootstrap.
class P2pGroupTestPeek {
  public:
    P2pGroupTestPeek(int gsize, int me) : g_(new P2pGroup()) {
        const size_t N = static_cast<size_t>(gsize);
        g_->gsize_ = gsize;
        g_->my_idx_ = me;
        g_->nlanes_ = kLanes;
        g_->nslots_ = kSlots;
        g_->slot_bytes_ = kSlotBytes;
        g_->flags_bytes_ = N * kLanes * 2 * 128;   // Create(): 128-byte flag stride
        g_->win_bytes_ = g_->flags_bytes_ + N * kLanes * kSlots * kSlotBytes;
        g_->peer_base_.resize(N);
        for (size_t i = 0; i < N; ++i) g_->peer_base_[i] = Fake<uint8_t>(i + 1);
        g_->my_base_ = g_->peer_base_[static_cast<size_t>(me)];
        g_->sent_.assign(N * kLanes, 0);
        g_->rcvd_.assign(N * kLanes, 0);
        g_->fused_sent_.assign(N * kLanes, 0);
        g_->fused_rcvd_.assign(N * kLanes, 0);
        g_->fanin_adds_.assign(kLanes, 0);
        g_->ctr_dev_ = Fake<uint64_t>(0x20);
        g_->abort_host_ = Fake<uint32_t>(0x21);
        g_->status_host_ = g_->abort_host_ + 1;
        g_->max_ticks_ = 300ull * 100000000ull;
        g_->hw_write_ = false;
    }
    ~P2pGroupTestPeek() { g_->my_base_ = nullptr; }   // the destructor returns early
    P2pGroup& operator*() { return *g_; }

  private:
    std::unique_ptr<P2pGroup> g_;
};

namespace {

struct Case {
    std::string name;
    int N;
    DataType dt;          // the request's dtype, not sch.dtype
    size_t wire_unit;     // QParams().WireBlockBytes(); unused without a plan
    std::function<ChunkExec(int)> make;   // the chunk of rank r
};

ChunkExec Plain(Schedule sch) {
    ChunkExec ce;
    ce.sch = std::move(sch);
    return ce;
}
// A compressed chunk as BuildChunks makes it: `seg_units` wire units per plan
// segment, the last block three elements short, 4-byte elements.
ChunkExec Planned(Schedule sch, size_t nseg, int r, size_t seg_units, size_t block,
                  QuantGather gather = QuantGather::NONE) {
    ChunkExec ce;
    ce.sch = std::move(sch);
    ce.qplan = MakeQuantPlan(ce.sch, nseg, static_cast<size_t>(r), seg_units * block - 3, 4, gather);
    return ce;
}

const char* DtName(DataType dt) {
    switch (dt) {
        case DataType::F32: return "f32";
        case DataType::BF16: return "bf16";
        case DataType::I32: return "i32";
        case DataType::I64: return "i64";
        default: return "dt";
    }
}

std::vector<Case> AllCases() {
    std::vector<Case> cs;
    const size_t MiB3 = 3u << 20;
    auto sz = [](bool large) { return large ? "large" : "small"; };
    // ring allreduce: fuse_into, fused and wide; I32 makes the fused and the
    // wide reduce launchers decline
    struct RingCfg { int N, stride; DataType dt; ReduceOp op; };
    const RingCfg rings[] = {
        {2, 1, DataType::F32, ReduceOp::SUM}, {2, 1, DataType::BF16, ReduceOp::MAX},
        {3, 1, DataType::F32, ReduceOp::SUM}, {3, 1, DataType::BF16, ReduceOp::MAX},
        {3, 2, DataType::F32, ReduceOp::SUM}, {3, 2, DataType::BF16, ReduceOp::MAX},
        {2, 1, DataType::I32, ReduceOp::SUM}};
    for (const RingCfg& c : rings)
        for (bool large : {false, true}) {
            const size_t n = static_cast<size_t>(c.N);
            const size_t count = large ? n * (MiB3 / DtypeSize(c.dt)) : 1000 * n + 1;
            cs.push_back({std::string("ring/n") + std::to_string(c.N) + "s" +
                              std::to_string(c.stride) + "/" + DtName(c.dt) + "/" + sz(large),
                          c.N, c.dt, 0, [=](int r) {
                              return Plain(BuildAllReduceRing(r, c.N, count, c.dt, c.op, c.stride));
                          }});
        }
    // RHD; a group that is no power of two gets the ring, as in BuildChunks
    for (int N : {4, 3})
        cs.push_back({"rhd/n" + std::to_string(N) + "/bf16/small", N, DataType::BF16, 0, [=](int r) {
                          return Plain((N & (N - 1)) == 0
                                           ? BuildAllReduceRHD(r, N, 4099, DataType::BF16, ReduceOp::SUM)
                                           : BuildAllReduceRing(r, N, 4099, DataType::BF16,
                                                                ReduceOp::SUM, 1));
                      }});
    // one-shot allreduce: the fan path, and what sends it to the generic loop
    struct DirectCfg { const char* tag; int N; DataType dt; size_t count; };
    const DirectCfg directs[] = {
        {"small", 2, DataType::F32, 1025},  {"small", 2, DataType::BF16, 1025},
        {"small", 4, DataType::F32, 1025},  {"small", 4, DataType::BF16, 1025},
        {"small", 4, DataType::I32, 1025},                  // dtype not covered
        {"above_fused", 2, DataType::F32, (3u << 19) / 4},  // 1.5 MiB
        {"small", 10, DataType::F32, 1025}};                // more than 8 peers
    for (const DirectCfg& c : directs)
        cs.push_back({std::string("direct/n") + std::to_string(c.N) + "/" + DtName(c.dt) + "/" + c.tag,
                      c.N, c.dt, 0, [=](int r) {
                          return Plain(BuildAllReduceDirect(r, c.N, c.count, c.dt, ReduceOp::SUM));
                      }});
    // reduce-scatter: fuse_out, and with I64 its LaunchReduceOut fallback
    for (DataType dt : {DataType::F32, DataType::I64})
        for (bool large : {false, true}) {
            const size_t count = large ? MiB3 / DtypeSize(dt) : 1001;
            cs.push_back({std::string("rs/n3/") + DtName(dt) + "/" + sz(large), 3, dt, 0, [=](int r) {
                              return Plain(BuildReduceScatter(r, 3, count, dt, ReduceOp::SUM));
                          }});
        }
    // plain copy consume and trailing COPY ops
    cs.push_back({"ag/n3/small", 3, DataType::F32, 0,
                  [](int r) { return Plain(BuildAllGather(r, 3, 1001, DataType::F32)); }});
    cs.push_back({"bcast/n3/root1/small", 3, DataType::F32, 0,
                  [](int r) { return Plain(BuildBcast(r, 3, 1001, DataType::F32, 1)); }});
    cs.push_back({"a2a/n3/small", 3, DataType::F32, 0,
                  [](int r) { return Plain(BuildAlltoAll(r, 3, 1001, DataType::F32)); }});
    cs.push_back({"barrier/n3", 3, DataType::F32, 0, [](int r) { return Plain(BuildBarrier(r, 3)); }});
    // compressed schedules with their plans
    for (size_t block : {size_t(256), size_t(64)})
        for (bool large : {false, true}) {
            const size_t U = block + 8;
            const size_t seg = large ? (MiB3 + U - 1) / U : 5;   // units per segment
            const size_t flat = large ? 3 * seg : 16;            // units of a flat wire
            const std::string tail = "/n3/b" + std::to_string(block) + "/" + sz(large);
            cs.push_back({"ring_units" + tail, 3, DataType::F32, U, [=](int r) {
                              return Planned(BuildAllReduceRingUnits(r, 3, flat, U, block), 1, r,
                                             flat, block);
                          }});
            cs.push_back({"rs_units" + tail, 3, DataType::BF16, U, [=](int r) {
                              return Planned(BuildReduceScatterUnits(r, 3, seg, U, block), 3, r, seg,
                                             block);
                          }});
            cs.push_back({"rs_direct_units" + tail, 3, DataType::F32, U, [=](int r) {
                              return Planned(BuildReduceScatterDirectUnits(r, 3, seg, U, block), 3, r,
                                             seg, block);
                          }});
            cs.push_back({"ag_units" + tail, 3, DataType::BF16, U, [=](int r) {
                              return Planned(BuildAllGatherUnits(r, 3, seg, U, block), 3, r, seg,
                                             block, QuantGather::ASSIGN);
                          }});
            cs.push_back({"twoshot_units" + tail, 3, DataType::F32, U, [=](int r) {
                              return Planned(BuildAllReduceTwoShotUnits(r, 3, flat, U, block), 1, r,
                                             flat, block);
                          }});
        }
    // two units over three ranks: one rank owns nothing
    cs.push_back({"twoshot_units/n3/b256/2units", 3, DataType::F32, 264, [](int r) {
                      return Planned(BuildAllReduceTwoShotUnits(r, 3, 2, 264, 256), 1, r, 2, 256);
                  }});
    return cs;
}

std::string TraceRank(const Case& c, int r) {
    std::string out;
    g_kernel_trace = &out;
    P2pGroupTestPeek g(c.N, r);
    ChunkExec ce = c.make(r);
    const bool planned = ce.sch.quant_block > 0;
    // device_comm.cpp: a compressed chunk walks with SEND = RECV = its plan's
    // base and TMP = the plan's scratch region
    uint8_t* base = Fake<uint8_t>(0x32);
    const uint8_t* sbase = planned ? base : Fake<uint8_t>(0x30);
    uint8_t* rbase = planned ? base : Fake<uint8_t>(0x31);
    uint8_t* tmp = planned ? base + ce.qplan.scratch_off : base;
    for (size_t lane : {size_t(0), size_t(0), size_t(1)}) {
        out += "# lane " + std::to_string(lane) + "\n";
        (*g).IssueSchedule(c.dt, c.wire_unit, ce, lane, Fake<ihipStream_t>(0x40, lane), sbase,
                           rbase, tmp);
    }
    g_kernel_trace = nullptr;
    return out;
}

// The RCCL walker's local op, which no GPU of the pool can run: one call per
// op kind (and a COPY onto itself, which launches nothing).
std::vector<std::pair<std::string, std::string>> TraceLocalOps() {
    std::vector<std::pair<std::string, std::string>> res;
    hipStream_t s = Fake<ihipStream_t>(0x40);
    uint8_t* base = Fake<uint8_t>(0x32);
    uint8_t *d = Fake<uint8_t>(0x31, 4096), *src = Fake<uint8_t>(0x30, 8192);
    const QuantPlan none;
    ChunkExec two = Planned(BuildAllReduceTwoShotUnits(1, 3, 16, 264, 256), 1, 1, 16, 256);
    ChunkExec ring = Planned(BuildAllReduceRingUnits(1, 3, 16, 264, 256), 1, 1, 16, 256);
    auto run = [&](const char* name, const Step& st, uint8_t* dst, uint8_t* from,
                   const QuantPlan& plan, DataType dt, ReduceOp rop, size_t unit) {
        std::string out;
        g_kernel_trace = &out;
        LaunchLocalOp(st, dst, from, plan, base, dt, rop, unit, s, /*nt=*/true);
        g_kernel_trace = nullptr;
        res.emplace_back(name, out);
    };
    auto at = [&](const ChunkExec& ce, const BufRef& b) {
        return SpacePtr(b, base, base, base + ce.qplan.scratch_off);
    };
    Step st;
    st.local = Step::LocalOp::COPY;
    st.local_src.bytes = st.local_dst.bytes = 4004;
    run("localop/copy", st, d, src, none, DataType::F32, ReduceOp::SUM, 0);
    run("localop/copy_onto_itself", st, d, d, none, DataType::F32, ReduceOp::SUM, 0);
    st.local = Step::LocalOp::REDUCE;
    run("localop/reduce", st, d, src, none, DataType::BF16, ReduceOp::MAX, 0);
    for (const Step& q : ring.sch.steps)
        if (q.local == Step::LocalOp::REDUCE) {
            run("localop/quant_accum", q, at(ring, q.local_dst), at(ring, q.local_src), ring.qplan,
                DataType::F32, ReduceOp::SUM, 264);
            break;
        }
    for (const Step& q : two.sch.steps)
        if (q.local == Step::LocalOp::SUMQ)
            run("localop/sumq", q, at(two, q.local_dst), at(two, q.local_src), two.qplan,
                DataType::F32, ReduceOp::SUM, 264);
    return res;
}

void Report(const char* mode, const std::string& name, int r, const std::string& text) {
    uint64_t h = 14695981039346656037ull;
    size_t calls = 0;
    for (size_t i = 0; i < text.size(); ++i) {
        h = (h ^ static_cast<uint8_t>(text[i])) * 1099511628211ull;
        if ((i == 0 || text[i - 1] == '\n') && text[i] != ' ' && text[i] != '#') ++calls;
    }
    std::printf("fused_max_kb=%s %s r%d %zu %016llx\n", mode, name.c_str(), r, calls,
                static_cast<unsigned long long>(h));
}

}  // namespace
}  // namespace mlsl

int main(int argc, char** argv) {
    using namespace mlsl;
    const char* env = std::getenv("MLSL_P2P_FUSED_MAX_KB");
    const char* mode = env ? env : "unset";
    const char* dump = argc == 3 && !std::strcmp(argv[1], "--dump") ? argv[2] : nullptr;
    if (argc != 1 && !dump) {
        std::fprintf(stderr, "usage: %s [--dump CASE]\n", argv[0]);
        return 2;
    }
    bool found = false;
    for (const Case& c : AllCases())
        for (int r = 0; r < c.N; ++r) {
            if (dump && c.name != dump) continue;
            const std::string text = TraceRank(c, r);
            found = true;
            if (dump) std::printf("== %s r%d\n%s", c.name.c_str(), r, text.c_str());
            else Report(mode, c.name, r, text);
        }
    for (const auto& lo : TraceLocalOps()) {
        if (dump && lo.first != dump) continue;
        found = true;
        if (dump) std::printf("== %s\n%s", lo.first.c_str(), lo.second.c_str());
        else Report(mode, lo.first, 0, lo.second);
    }
    if (!found) {
        std::fprintf(stderr, "no such case: %s\n", dump);
        return 2;
    }
    return 0;
}
