#include "p2p_transport.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "../core/config.hpp"
#include "../core/log.hpp"
#include "../hip/kernels.hpp"
#include "bootstrap.hpp"
#include "context.hpp"
#include "device_local_op.hpp"
#include "group.hpp"
#include "request.hpp"

namespace mlsl {

#define HIP_CHECKP(cmd)                                                       \
    do {                                                                      \
        hipError_t e_ = (cmd);                                                \
        if (e_ != hipSuccess)                                                 \
            MLSL_THROW(std::string("HIP error (p2p): ") +                     \
                       hipGetErrorString(e_));                                \
    } while (0)

namespace {
// Flag mailboxes are 128-byte-strided so flags written by different peers
// never share a cache line (remote stores would otherwise ping-pong lines
// between GPUs over xGMI).
constexpr size_t kFlagStride = 128;
// Sub-messages at or below this ride the fully-fused bounded-grid kernels
// (one launch per side); larger ones use wide kernels with separate 1-wg
// waits so the payload kernels never spin. Tunable: MLSL_P2P_FUSED_MAX_KB.
size_t FusedMaxBytes() {
    static const size_t v = [] {
        if (const char* e = std::getenv("MLSL_P2P_FUSED_MAX_KB")) {
            long long kb = std::atoll(e);
            if (kb >= 0) return static_cast<size_t>(kb) * 1024;
        }
        return static_cast<size_t>(1u << 20);
    }();
    return v;
}
std::mutex g_issue_mu;  // enqueue-order == counter-order per group

struct WireHandle {
    hipIpcMemHandle_t h;
    int valid;
};
}  // namespace

std::unique_ptr<P2pGroup> P2pGroup::Create(ProcessGroup* g, size_t nlanes,
                                           size_t nslots, size_t slot_bytes) {
    Context& ctx = Context::Get();
    auto pg = std::unique_ptr<P2pGroup>(new P2pGroup());
    pg->gsize_ = g->Size();
    pg->my_idx_ = g->MyIdx();
    pg->nlanes_ = nlanes;
    pg->nslots_ = nslots;
    pg->slot_bytes_ = slot_bytes;
    const size_t N = static_cast<size_t>(pg->gsize_);
    pg->flags_bytes_ = N * nlanes * 2 * kFlagStride;
    pg->win_bytes_ = pg->flags_bytes_ + N * nlanes * nslots * slot_bytes;

    WireHandle mine{};
    std::memset(&mine, 0, sizeof(mine));
    const bool member = g->IsMember() && g->Size() > 1;
    if (member) {
        HIP_CHECKP(hipMalloc(reinterpret_cast<void**>(&pg->my_base_),
                             pg->win_bytes_));
        // Zero ONLY the flag region: flags/acks are accessed exclusively
        // with system-scope atomics (coherent). The slot payload area is
        // deliberately left untouched — a local memset would leave this
        // process's caches holding zero lines that can shadow the peer's
        // later payload stores (cold-box page-scrub lines shadowed arrivals
        // the same way; slots are fully overwritten before every consume,
        // so they never need initialization).
        HIP_CHECKP(hipMemset(pg->my_base_, 0, pg->flags_bytes_));
        HIP_CHECKP(hipIpcGetMemHandle(&mine.h, pg->my_base_));
        mine.valid = 1;
        HIP_CHECKP(hipHostMalloc(reinterpret_cast<void**>(&pg->abort_host_),
                                 2 * sizeof(uint32_t)));
        pg->status_host_ = pg->abort_host_ + 1;
        pg->abort_host_[0] = 0;
        pg->status_host_[0] = 0;
        const int tmo = GlobalConfig().timeout_sec;
        pg->max_ticks_ = static_cast<uint64_t>(tmo > 0 ? tmo : 300) * 100000000ull;
    }

    // Same exchange pattern as the RCCL unique-id path: world-wide
    // bootstrap allgather, indexed by world rank.
    std::vector<WireHandle> all(static_cast<size_t>(ctx.Boot()->Size()));
    ctx.Boot()->Allgather(&mine, sizeof(WireHandle), all.data());
    if (member) {
        pg->peer_base_.assign(N, nullptr);
        pg->sent_.assign(N * nlanes, 0);
        pg->rcvd_.assign(N * nlanes, 0);
        pg->fused_sent_.assign(N * nlanes, 0);
        pg->fused_rcvd_.assign(N * nlanes, 0);
        pg->fanin_adds_.assign(nlanes, 0);
        const size_t nctr = 2 * N * nlanes + nlanes;
        HIP_CHECKP(hipMalloc(reinterpret_cast<void**>(&pg->ctr_dev_),
                             nctr * sizeof(uint64_t)));
        HIP_CHECKP(hipMemset(pg->ctr_dev_, 0, nctr * sizeof(uint64_t)));
        for (int i = 0; i < pg->gsize_; ++i) {
            if (i == pg->my_idx_) {
                pg->peer_base_[i] = pg->my_base_;
                continue;
            }
            const WireHandle& wh = all[static_cast<size_t>(g->WorldRank(i))];
            MLSL_CHECK(wh.valid, "p2p window handle missing for a group peer");
            void* p = nullptr;
            HIP_CHECKP(hipIpcOpenMemHandle(&p, wh.h,
                                           hipIpcMemLazyEnablePeerAccess));
            pg->peer_base_[i] = static_cast<uint8_t*>(p);
        }
        // hipStreamWriteValue64 publishes measured SLOWER than the 1-wg
        // SetFlag kernel in a same-box A/B (4 KiB: 45 vs 39 us; 256 MiB
        // ring: 310 vs 353 GB/s — the write packet stalls the queue), so
        // the HW path is opt-in: MLSL_P2P_HW_WRITE=1.
        const char* hw_env = std::getenv("MLSL_P2P_HW_WRITE");
        const bool hw_allowed = hw_env && std::atoi(hw_env) != 0;
        // Probe hipStreamWriteValue64 on window memory: if the runtime
        // accepts it, publishes/acks ride the queue as packets (no kernel
        // launch). The value written here is 0 == the initial state.
        if (hw_allowed) {
            hipStream_t ps;
            if (hipStreamCreateWithFlags(&ps, hipStreamNonBlocking) == hipSuccess) {
                hipError_t we = hipStreamWriteValue64(
                    ps, pg->MyInFlag(pg->my_idx_, 0), 0ull, 0);
                if (we == hipSuccess && hipStreamSynchronize(ps) == hipSuccess)
                    pg->hw_write_ = true;
                else
                    (void)hipGetLastError();
                (void)hipStreamDestroy(ps);
            }
        }
        MLSL_LOG(DEBUG,
                 "p2p group ready: size=%d lanes=%zu slots=%zu slot_bytes=%zu "
                 "window=%zu MiB hw_write=%d",
                 pg->gsize_, nlanes, nslots, slot_bytes,
                 pg->win_bytes_ >> 20, (int)pg->hw_write_);
    }
    return pg;
}

P2pGroup::~P2pGroup() {
    if (!my_base_) return;
    // Unblock any in-flight wait kernels, let the device drain, then unmap.
    if (abort_host_) abort_host_[0] = 1;
    (void)hipDeviceSynchronize();
    for (int i = 0; i < gsize_; ++i)
        if (peer_base_[i] && i != my_idx_)
            (void)hipIpcCloseMemHandle(peer_base_[i]);
    (void)hipFree(my_base_);
    if (ctr_dev_) (void)hipFree(ctr_dev_);
    if (abort_host_) (void)hipHostFree(abort_host_);
}

bool P2pGroup::Healthy() const {
    return !status_host_ ||
           __atomic_load_n(status_host_, __ATOMIC_ACQUIRE) == 0;
}

void P2pGroup::Abort() {
    if (abort_host_) __atomic_store_n(abort_host_, 1u, __ATOMIC_RELEASE);
}

// --- window geometry -------------------------------------------------------
// Window of owner o: [flags][data]. Flag pair for (src s, lane l) at
// (s*nlanes+l)*2*kFlagStride: in_flag then ack_flag. in_flag = number of
// slot-messages s has pushed to o (written by s). ack_flag = number of
// slot-messages s has CONSUMED of those o pushed to s (also written by s).
// Data slot (s, l, k): payload staging for s -> o traffic.

uint8_t* P2pGroup::MySlot(int src, size_t lane, size_t slot) const {
    return my_base_ + flags_bytes_ +
           (((static_cast<size_t>(src) * nlanes_ + lane) * nslots_) + slot) *
               slot_bytes_;
}
uint8_t* P2pGroup::PeerSlot(int peer, size_t lane, size_t slot) const {
    return peer_base_[peer] + flags_bytes_ +
           (((static_cast<size_t>(my_idx_) * nlanes_ + lane) * nslots_) + slot) *
               slot_bytes_;
}
void* P2pGroup::MyInFlag(int src, size_t lane) const {
    return my_base_ + (static_cast<size_t>(src) * nlanes_ + lane) * 2 * kFlagStride;
}
void* P2pGroup::MyAckFlag(int peer, size_t lane) const {
    return my_base_ +
           (static_cast<size_t>(peer) * nlanes_ + lane) * 2 * kFlagStride +
           kFlagStride;
}
void* P2pGroup::PeerInFlag(int peer, size_t lane) const {
    return peer_base_[peer] +
           (static_cast<size_t>(my_idx_) * nlanes_ + lane) * 2 * kFlagStride;
}
void* P2pGroup::PeerAckFlag(int peer, size_t lane) const {
    return peer_base_[peer] +
           (static_cast<size_t>(my_idx_) * nlanes_ + lane) * 2 * kFlagStride +
           kFlagStride;
}

void P2pGroup::PublishFlag(void* mbox, uint64_t val, hipStream_t s) {
    if (hw_write_) {
        if (hipStreamWriteValue64(s, mbox, val, 0) == hipSuccess) return;
        (void)hipGetLastError();
        hw_write_ = false;  // runtime changed its mind: kernels from now on
    }
    LaunchSetFlag(mbox, val, s);
}

// --- transport ops ---------------------------------------------------------

namespace {
// How a step's receive is consumed. The fusion cases: the received data IS
// the local op's source (ring/RHD reduce), or the local op targets the recv
// range (reduce-scatter's out-of-place accumulate). Both are handled per
// sub-message; any other local op runs unfused after the phase's traffic.
enum class Consume { COPY, REDUCE_INTO, REDUCE_OUT };

bool SameRef(const BufRef& a, const BufRef& b) {
    return a.space == b.space && a.off == b.off && a.bytes == b.bytes;
}
bool HasRecv(const Step& st) { return st.recv_peer >= 0 && st.recv.bytes > 0; }
Consume ConsumeOf(const Step& st) {
    if (st.local != Step::LocalOp::REDUCE) return Consume::COPY;
    if (SameRef(st.local_src, st.recv)) return Consume::REDUCE_INTO;
    if (SameRef(st.local_dst, st.recv) && st.local_src.bytes == st.recv.bytes)
        return Consume::REDUCE_OUT;
    return Consume::COPY;
}

// Adaptive sub-message size: ~8 sub-messages per transfer (pipelines DMA
// against the consumer's reduce) but never below 4 MiB (each wide-path
// sub-message costs ~5 kernel launches) and never above the slot.
// Sender and receiver derive the identical size from the transfer length,
// so the slot partition always agrees.
size_t SubSize(size_t bytes, size_t unit, size_t msg_max) {
    size_t v = std::max<size_t>((bytes + 7) / 8, std::min<size_t>(4u << 20, msg_max));
    v = std::min(v, msg_max);
    v = (v / unit) * unit;
    if (v < unit) v = unit;
    return std::min(v, msg_max);
}
}  // namespace

// What one IssueSchedule call holds fixed for its stages.
struct P2pGroup::Walk {
    const Schedule& sch;
    DataType dtype;
    size_t es, unit, blk;   // element bytes; sub-message granule; quant block (0: not compressed)
    size_t msg_max;         // the slot, rounded down to whole units
    size_t lane;
    hipStream_t s;
    const uint8_t* sbase;
    uint8_t *rbase, *tmp;
    bool Quant() const { return blk > 0; }
    uint8_t* Ptr(const BufRef& b) const { return SpacePtr(b, sbase, rbase, tmp); }
    // Sub-message k of a `bytes` transfer: false past its end.
    bool Sub(size_t bytes, size_t k, size_t* off, size_t* n) const {
        const size_t sub = SubSize(bytes, unit, msg_max);
        *off = k * sub;
        if (*off >= bytes) return false;
        *n = std::min(sub, bytes - *off);
        return true;
    }
    size_t NumSubs(size_t bytes) const {
        const size_t sub = SubSize(bytes, unit, msg_max);
        return (bytes + sub - 1) / sub;
    }
};

P2pGroup::Edge P2pGroup::Advance(std::vector<uint64_t>& seqs, int peer, size_t lane) const {
    const size_t idx = static_cast<size_t>(peer) * nlanes_ + lane;
    const uint64_t seq = ++seqs[idx];
    return {seq, (seq - 1) % nslots_, idx};
}

XferPoll P2pGroup::Poll(const void* mbox, uint64_t target) const {
    return {mbox, target, abort_host_, status_host_, max_ticks_};
}

// One-shot (direct) allreduce fast path: the whole exchange phase becomes
// TWO kernels — a fan-out pushing the payload to every peer and a fan-in
// waiting all arrivals and reducing them in a single pass over dst. Declines
// (false, nothing issued) for large payloads, >8 peers or uncovered dtypes:
// the generic loop takes the phase then.
bool P2pGroup::TryFanPhase(const Walk& w, int phase) {
    if (!w.sch.one_shot || phase != 1 || w.Quant()) return false;
    std::vector<const Step*> fan;
    for (const auto& st : w.sch.steps)
        if (st.phase == 1) fan.push_back(&st);
    const size_t B = fan.empty() ? 0 : fan[0]->send.bytes;
    const bool covered = w.dtype == DataType::F32 || w.dtype == DataType::BF16;
    if (fan.empty() || fan.size() > 8 || B == 0 || B > w.msg_max || B > FusedMaxBytes() ||
        !covered)
        return false;
    const XferPoll ab = Poll(nullptr, 0);
    FanPeer sp[8], rp[8];
    const int np = static_cast<int>(fan.size());
    for (int i = 0; i < np; ++i) {
        const int peer = fan[i]->send_peer;
        const Edge se = NextSend(peer, w.lane);
        sp[i].slot = PeerSlot(peer, w.lane, se.slot);
        sp[i].flag = PeerInFlag(peer, w.lane);
        sp[i].flag_val = se.seq;
        sp[i].wait_mbox = se.seq > nslots_ ? MyAckFlag(peer, w.lane) : nullptr;
        sp[i].wait_target = se.seq - nslots_;
        sp[i].ctr = ctr_dev_ + se.idx;
        sp[i].ctr_target = fused_sent_[se.idx] += static_cast<uint64_t>(FanOutWgsPerPeer(np));
        const Edge re = NextRecv(peer, w.lane);
        rp[i].slot = MySlot(peer, w.lane, re.slot);
        rp[i].flag = PeerAckFlag(peer, w.lane);
        rp[i].flag_val = re.seq;
        rp[i].wait_mbox = MyInFlag(peer, w.lane);
        rp[i].wait_target = re.seq;
        rp[i].ctr = nullptr;
        rp[i].ctr_target = 0;
    }
    LaunchFanOutSend(w.Ptr(fan[0]->send), B, sp, np, &ab, w.s);
    uint64_t* fctr = ctr_dev_ + 2 * static_cast<size_t>(gsize_) * nlanes_ + w.lane;
    const bool ok = LaunchFanInReduce(w.Ptr(fan[0]->local_dst), B / w.es, w.dtype, w.sch.rop, rp,
                                      np, fctr, fanin_adds_[w.lane] += kXferFusedGrid, &ab, w.s);
    MLSL_CHECK(ok, "fan-in dtype dispatch failed");
    return true;
}

// Sub-message k of a step's send (nothing past the transfer's end).
void P2pGroup::SendSub(const Walk& w, const Step& st, size_t k) {
    size_t off, n;
    if (!w.Sub(st.send.bytes, k, &off, &n)) return;
    const int peer = st.send_peer;
    const Edge e = NextSend(peer, w.lane);
    uint8_t* slot = PeerSlot(peer, w.lane, e.slot);
    // backpressure: the slot is free once the peer has acked its last use
    const void* ack = e.seq > nslots_ ? MyAckFlag(peer, w.lane) : nullptr;
    if (n <= FusedMaxBytes()) {
        // Small sub-message: ONE bounded-grid kernel does the backpressure
        // poll, the slot copy and the publish (32 workgroups can never
        // starve the peer — the full-device fused variant deadlocked; see
        // below).
        const XferPoll bp = Poll(ack, e.seq - nslots_);
        LaunchXferSendFused(slot, w.Ptr(st.send) + off, n, ack ? &bp : nullptr,
                            ctr_dev_ + e.idx, fused_sent_[e.idx] += kXferFusedGrid,
                            PeerInFlag(peer, w.lane), e.seq, w.s);
        return;
    }
    // Backpressure (slot reuse) as a SEPARATE 1-wg wait kernel: a poll fused
    // into a FULL-DEVICE copy kernel deadlocked two same-device ranks — each
    // rank's spinner starved the peer's consumer kernel of CUs (measured at
    // 256 MiB world-2). The 1-wg wait always co-schedules.
    if (ack)
        LaunchWaitFlag(ack, e.seq - nslots_, abort_host_, status_host_, max_ticks_, w.s);
    LaunchXferCopy(slot, w.Ptr(st.send) + off, n, nullptr, w.s);
    PublishFlag(PeerInFlag(peer, w.lane), e.seq, w.s);
}

// Sub-message k of a step's receive, consumed as ConsumeOf(st) says.
void P2pGroup::RecvSub(const Walk& w, const Step& st, size_t k) {
    const Consume c = ConsumeOf(st);
    size_t off, n;
    if (!w.Sub(st.recv.bytes, k, &off, &n)) return;
    const int peer = st.recv_peer;
    const Edge e = NextRecv(peer, w.lane);
    const uint8_t* sl = MySlot(peer, w.lane, e.slot);
    void* arrived = MyInFlag(peer, w.lane);
    void* ack = PeerAckFlag(peer, w.lane);
    const size_t qelems = w.Quant() ? (n / w.unit) * w.blk : 0;
    if (n <= FusedMaxBytes()) {
        // Small sub-message: the wait, the consume and the ack in one
        // bounded-grid kernel.
        const XferPoll wp = Poll(arrived, e.seq);
        uint64_t* rctr = ctr_dev_ + static_cast<size_t>(gsize_) * nlanes_ + e.idx;
        if (w.Quant() && c == Consume::REDUCE_INTO) {
            // compressed-domain accumulate with the wait fused in
            LaunchXferRecvQuantAccum(w.Ptr(st.local_dst) + off, sl, qelems, w.blk, &wp, rctr,
                                     fused_rcvd_[e.idx] += kXferFusedGrid, ack, e.seq, w.s);
            return;
        }
        if (!w.Quant() || c == Consume::COPY) {
            // COPY (byte copy) is dtype-agnostic, so quant AG forwards ride
            // it too
            const FusedConsume mode = c == Consume::REDUCE_INTO  ? FusedConsume::REDUCE
                                      : c == Consume::REDUCE_OUT ? FusedConsume::REDUCE_OUT
                                                                 : FusedConsume::COPY;
            uint8_t* d = w.Ptr(c == Consume::REDUCE_INTO ? st.local_dst : st.recv) + off;
            const uint8_t* o = c == Consume::REDUCE_OUT ? w.Ptr(st.local_src) + off : nullptr;
            if (LaunchXferRecvFused(d, sl, o, c == Consume::COPY ? n : n / w.es, w.dtype,
                                    w.sch.rop, mode, &wp, rctr,
                                    fused_rcvd_[e.idx] += kXferFusedGrid, ack, e.seq, w.s))
                return;
            fused_rcvd_[e.idx] -= kXferFusedGrid;  // dtype not covered: nothing was launched
        }
    }
    // Arrival wait as a 1-wg kernel (same deadlock avoidance as the sender
    // backpressure), then the wide consume kernel, then the ack.
    LaunchWaitFlag(arrived, e.seq, abort_host_, status_host_, max_ticks_, w.s);
    switch (c) {
        case Consume::COPY:
            LaunchXferCopy(w.Ptr(st.recv) + off, sl, n, nullptr, w.s);
            break;
        case Consume::REDUCE_INTO: {
            uint8_t* d = w.Ptr(st.local_dst) + off;
            if (w.Quant())
                LaunchQuantAccum(d, sl, qelems, w.blk, w.s);
            else if (!LaunchXferReduce(d, sl, nullptr, n / w.es, w.dtype, w.sch.rop, nullptr, w.s))
                LaunchReduce(d, sl, n / w.es, w.dtype, w.sch.rop, w.s);
            break;
        }
        case Consume::REDUCE_OUT: {
            uint8_t* d = w.Ptr(st.recv) + off;
            const uint8_t* o = w.Ptr(st.local_src) + off;
            if (w.Quant()) {
                // acc = slot, then acc += local_src slice
                LaunchCopyVariant(d, sl, n, false, w.s);
                LaunchQuantAccum(d, o, qelems, w.blk, w.s);
            } else if (!LaunchXferReduce(d, sl, o, n / w.es, w.dtype, w.sch.rop, nullptr, w.s)) {
                LaunchReduceOut(d, sl, o, n / w.es, w.dtype, w.sch.rop, w.s);
            }
            break;
        }
    }
    PublishFlag(ack, e.seq, w.s);
}

void P2pGroup::IssueSchedule(DataType dtype, size_t wire_unit, ChunkExec& ce, size_t lane,
                             hipStream_t s, const uint8_t* sbase, uint8_t* rbase,
                             uint8_t* tmp) {
    std::lock_guard<std::mutex> lk(g_issue_mu);
    MLSL_CHECK(lane < nlanes_, "p2p lane out of range");
    const size_t es = DtypeSize(dtype);
    const size_t blk = ce.sch.quant_block;
    const size_t unit = blk > 0 ? wire_unit : es;
    const Walk w{ce.sch, dtype, es,    unit,  blk, (slot_bytes_ / unit) * unit,
                 lane,   s,     sbase, rbase, tmp};
    MLSL_CHECK(w.msg_max > 0, "p2p slot smaller than one element/block");

    for (int phase = 0; phase < ce.sch.num_phases; ++phase) {
        if (TryFanPhase(w, phase)) continue;
        // Collect this phase's send and recv jobs, then interleave their
        // sub-messages round-robin. The interleave is what makes the
        // bounded slot ring deadlock-free: a sender blocked on backpressure
        // (ack >= seq-kSlots) is guaranteed that its OWN next consume —
        // which is what its upstream neighbor is waiting on — was already
        // enqueued at the previous sub-message index. Issuing all sends of
        // a phase before any recv would cycle-deadlock the ring whenever a
        // segment needs more sub-messages than there are slots.
        std::vector<const Step*> sends, recvs;
        size_t max_msgs = 0;
        for (const auto& st : ce.sch.steps) {
            if (st.phase != phase) continue;
            if (st.send_peer >= 0 && st.send.bytes > 0) {
                MLSL_CHECK(st.send_peer != my_idx_, "p2p self-send in schedule");
                sends.push_back(&st);
                max_msgs = std::max(max_msgs, w.NumSubs(st.send.bytes));
            }
            if (HasRecv(st)) {
                MLSL_CHECK(st.recv_peer != my_idx_, "p2p self-recv in schedule");
                recvs.push_back(&st);
                max_msgs = std::max(max_msgs, w.NumSubs(st.recv.bytes));
            }
        }
        for (size_t k = 0; k < max_msgs; ++k) {
            for (const Step* st : sends) SendSub(w, *st, k);
            for (const Step* st : recvs) RecvSub(w, *st, k);
        }
        // Unfused local ops (pure copy steps, or reduce with unrelated
        // source/dest geometry) run after the phase's traffic, step order.
        for (const auto& st : ce.sch.steps) {
            if (st.phase != phase || st.local == Step::LocalOp::NONE) continue;
            if (st.local_dst.bytes == 0) continue;  // zero-length segment
            if (HasRecv(st) && ConsumeOf(st) != Consume::COPY) continue;  // done per sub-message
            // a compressed chunk's sbase is its plan's base; the arrival
            // slots were filled by this stream's consume kernels above
            LaunchLocalOp(st, w.Ptr(st.local_dst), w.Ptr(st.local_src), ce.qplan,
                          const_cast<uint8_t*>(sbase), dtype, ce.sch.rop, wire_unit, s,
                          /*nt=*/false);
        }
    }
}

}  // namespace mlsl
