// RCCL/HIP device transport: per-group communicators (one per channel,
// each on its own HIP stream), fused RCCL collectives as the baseline path,
// and schedule-driven ncclSend/ncclRecv + local-reduce HIP kernel pipelines
// as the custom path (MLSL_ALLREDUCE_ALGO=ring|rhd).
//
// Re-designs the reference process-mode backend (src/comm_ep.cpp): endpoint
// servers -> channel streams; shm heap + ReplaceIn/Out staging -> HBM
// buffers (hipMalloc) used directly; MPI_I* -> RCCL enqueues; MPI_Test
// polling loop -> hipEventQuery from the progress thread.
#include "device_comm.hpp"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <unistd.h>
#include <unordered_map>
#include <vector>

#include "../core/config.hpp"
#include "../core/log.hpp"
#include "device_pool.hpp"
#include "../hip/kernels.hpp"
#include "bootstrap.hpp"
#include "context.hpp"
#include "p2p_transport.hpp"
#include "quant.hpp"
#include "device_local_op.hpp"
#include "device_state.hpp"
#include "group.hpp"
#include "request.hpp"

namespace mlsl {

#define HIP_CHECKD(cmd)                                                       \
    do {                                                                      \
        hipError_t e_ = (cmd);                                                \
        if (e_ != hipSuccess)                                                 \
            MLSL_THROW(std::string("HIP error: ") + hipGetErrorString(e_));   \
    } while (0)

#define NCCL_CHECK(cmd)                                                       \
    do {                                                                      \
        ncclResult_t r_ = (cmd);                                              \
        if (r_ != ncclSuccess)                                                \
            MLSL_THROW(std::string("RCCL error: ") + ncclGetErrorString(r_)); \
    } while (0)

DeviceReqState::~DeviceReqState() {
    if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
    for (hipEvent_t e : events)
        if (e) (void)hipEventDestroy(e);
    if (dep_event) (void)hipEventDestroy(dep_event);
    if (t0_event) (void)hipEventDestroy(t0_event);
    // Return scratch to the HBM pool while the runtime is alive; fall back
    // to hipFree during teardown.
    DeviceRuntime* rt = Context::Initialized() ? Context::Get().Device() : nullptr;
    auto rel = [&](void* p) {
        if (!p) return;
        if (rt) rt->FreeDevice(p);
        else (void)hipFree(p);
    };
    rel(tmp_dev);
    rel(stage_send);
    rel(stage_recv);
    rel(seg_dev);
    if (seg_ptrs_pin) (void)hipHostFree(seg_ptrs_pin);
    if (pin_send) (void)hipHostFree(pin_send);
    if (pin_recv) (void)hipHostFree(pin_recv);
}

namespace {

ncclDataType_t ToNccl(DataType dt) {
    switch (dt) {
        case DataType::F32: return ncclFloat32;
        case DataType::F64: return ncclFloat64;
        case DataType::U8: return ncclUint8;
        case DataType::BF16: return ncclBfloat16;
        case DataType::F16: return ncclFloat16;
        case DataType::I32: return ncclInt32;
        case DataType::I64: return ncclInt64;
    }
    return ncclFloat32;
}

ncclRedOp_t ToNcclOp(ReduceOp op) {
    switch (op) {
        case ReduceOp::SUM: return ncclSum;
        case ReduceOp::MIN: return ncclMin;
        case ReduceOp::MAX: return ncclMax;
    }
    return ncclSum;
}

// Per-group device communicators: `channels` RCCL comms, each with its own
// stream — chunk c of a request runs on channel c % channels, so chunks of
// one large message progress on independent RCCL rings over distinct xGMI
// link schedules (the endpoint-server fan-out analog).
struct GroupComms {
    std::vector<ncclComm_t> comms;
    std::vector<hipStream_t> streams;
    // High-priority lane for MLSL_MSG_PRIORITY traffic (fresh urgent
    // gradients overtake queued bulk work — stream-priority analog of the
    // reference's newest-first server scan).
    hipStream_t prio_stream = nullptr;
    ncclComm_t prio_comm = nullptr;
    // IPC window transport (comm/p2p_transport.hpp): set instead of comms
    // when the runtime decided on p2p (several ranks on one device, or
    // MLSL_DEVICE_TRANSPORT=p2p). Streams above are still the lanes.
    std::unique_ptr<P2pGroup> p2p;
};

class HipRuntime;
HipRuntime* g_runtime = nullptr;

class HipRuntime : public DeviceRuntime {
  public:
    HipRuntime(int device_id) : device_id_(device_id) {
        HIP_CHECKD(hipSetDevice(device_id_));
        // HBM pool: cache up to MLSL_HEAP_SIZE_MB of freed blocks
        // (0 = unlimited cache; 288 GB per GPU makes caching the default).
        const size_t heap_mb = GlobalConfig().heap_mb;
        pool_ = std::make_unique<DevicePool>(heap_mb * 1024 * 1024);
    }

    ~HipRuntime() override {
        for (auto& kv : group_comms_) {
            for (auto c : kv.second.comms) ncclCommDestroy(c);
            for (auto s : kv.second.streams) (void)hipStreamDestroy(s);
            if (kv.second.prio_comm) ncclCommDestroy(kv.second.prio_comm);
            if (kv.second.prio_stream) (void)hipStreamDestroy(kv.second.prio_stream);
        }
        g_runtime = nullptr;
    }

    int DeviceId() const override { return device_id_; }

    void SetComputeStream(void* stream) override {
        compute_stream_ = static_cast<hipStream_t>(stream);
    }
    void* ComputeStream() const override { return compute_stream_; }

    void* AllocDevice(size_t bytes) override { return pool_->Alloc(bytes); }

    void FreeDevice(void* p) override { pool_->Free(p); }

    void Synchronize() override { HIP_CHECKD(hipDeviceSynchronize()); }

    std::string Name() const override {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device_id_) == hipSuccess)
            return std::string("hip:") + prop.gcnArchName;
        return "hip:?";
    }

    bool UsesP2p() const override { return use_p2p_; }

    // Transport decision, made exactly once and identically on every rank
    // (collective over the world bootstrap): RCCL refuses two ranks of one
    // communicator on the same device ("Duplicate GPU detected" — verified
    // on this pool), so when any device is shared by several world ranks
    // the IPC window transport takes over for ALL groups. Env override:
    // MLSL_DEVICE_TRANSPORT=rccl|p2p.
    void DecideTransport() {
        if (transport_decided_) return;
        transport_decided_ = true;
        const std::string& want = GlobalConfig().device_transport;
        Context& ctx = Context::Get();
        struct HostDev { uint64_t host; int dev; };
        HostDev mine{0, device_id_};
        char hn[256] = {0};
        (void)gethostname(hn, sizeof(hn) - 1);
        for (const char* p = hn; *p; ++p) mine.host = mine.host * 131 + *p;
        std::vector<HostDev> all(static_cast<size_t>(ctx.Boot()->Size()));
        ctx.Boot()->Allgather(&mine, sizeof(HostDev), all.data());
        bool shared = false;
        for (size_t i = 0; i < all.size() && !shared; ++i)
            for (size_t j = i + 1; j < all.size(); ++j)
                if (all[i].host == all[j].host && all[i].dev == all[j].dev) {
                    shared = true;
                    break;
                }
        if (want == "p2p") use_p2p_ = true;
        else if (want == "rccl") use_p2p_ = false;
        else use_p2p_ = shared;
        if (use_p2p_)
            MLSL_LOG(INFO, "device transport: IPC p2p windows (%s)",
                     want == "p2p" ? "forced" : "shared-device layout");
    }

    // Collective over the WORLD: unique-id / window-handle exchange runs on
    // the bootstrap; only group members init comms / map windows.
    void EnsureGroupComms(ProcessGroup* g) override {
        if (group_comms_.count(g->Uid())) return;
        DecideTransport();
        Context& ctx = Context::Get();
        const Config& cfg = GlobalConfig();
        const size_t nch = cfg.num_channels;
        if (use_p2p_) {
            GroupComms gc;
            const size_t nlanes = nch + (cfg.msg_priority ? 1 : 0);
            gc.p2p = P2pGroup::Create(g, nlanes, cfg.p2p_slots,
                                      cfg.p2p_slot_mb << 20);
            if (g->IsMember() && g->Size() > 1) {
                for (size_t ch = 0; ch < nch; ++ch) {
                    hipStream_t s;
                    HIP_CHECKD(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
                    gc.streams.push_back(s);
                }
                if (cfg.msg_priority) {
                    int lo = 0, hi = 0;
                    HIP_CHECKD(hipDeviceGetStreamPriorityRange(&lo, &hi));
                    HIP_CHECKD(hipStreamCreateWithPriority(
                        &gc.prio_stream, hipStreamNonBlocking, hi));
                }
            } else {
                gc.p2p.reset();  // non-members keep no window state
            }
            group_comms_.emplace(g->Uid(), std::move(gc));
            MLSL_LOG(DEBUG, "p2p device comms ready for group uid=%d size=%d "
                     "lanes=%zu", g->Uid(), g->Size(), nlanes);
            return;
        }
        GroupComms gc;
        // Subgroups SPLIT the world communicators instead of paying a full
        // ncclCommInitRank per group (a Distribution(4,2) on 8 GPUs would
        // otherwise re-bootstrap RCCL per color). Colors are the group's
        // lowest world rank — unique across the disjoint groups of one
        // collective creation. World (and any group while the world comms
        // don't exist yet) takes the init path.
        GroupComms* wc = nullptr;
        const bool is_world = g == ctx.World();
        if (!is_world) {
            auto wit = group_comms_.find(ctx.World()->Uid());
            if (wit != group_comms_.end() && wit->second.comms.size() == nch)
                wc = &wit->second;
        }
        if (wc) {
            const int color = g->IsMember() && g->Size() > 1
                                  ? g->WorldRank(0)
                                  : NCCL_SPLIT_NOCOLOR;
            const int key = g->IsMember() ? g->MyIdx() : 0;
            for (size_t ch = 0; ch < nch; ++ch) {
                ncclComm_t sub = nullptr;
                NCCL_CHECK(ncclCommSplit(wc->comms[ch], color, key, &sub, nullptr));
                if (color != NCCL_SPLIT_NOCOLOR && sub) {
                    hipStream_t s;
                    HIP_CHECKD(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
                    gc.comms.push_back(sub);
                    gc.streams.push_back(s);
                }
            }
        } else {
            for (size_t ch = 0; ch < nch; ++ch) {
                ncclUniqueId id{};
                if (g->IsMember() && g->MyIdx() == 0) NCCL_CHECK(ncclGetUniqueId(&id));
                std::vector<ncclUniqueId> all(static_cast<size_t>(ctx.Boot()->Size()));
                ctx.Boot()->Allgather(&id, sizeof(ncclUniqueId), all.data());
                if (g->IsMember() && g->Size() > 1) {
                    ncclUniqueId gid = all[static_cast<size_t>(g->WorldRank(0))];
                    ncclComm_t comm;
                    NCCL_CHECK(ncclCommInitRank(&comm, g->Size(), gid, g->MyIdx()));
                    hipStream_t s;
                    HIP_CHECKD(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
                    gc.comms.push_back(comm);
                    gc.streams.push_back(s);
                }
            }
        }
        if (GlobalConfig().msg_priority) {
            // The bootstrap Allgather is collective over the WORLD — every
            // rank must participate (non-members contribute a zero id, as in
            // the channel loop above), else a subgroup with non-member ranks
            // desyncs the bootstrap stream.
            ncclUniqueId id{};
            if (g->IsMember() && g->MyIdx() == 0) NCCL_CHECK(ncclGetUniqueId(&id));
            std::vector<ncclUniqueId> all(static_cast<size_t>(ctx.Boot()->Size()));
            ctx.Boot()->Allgather(&id, sizeof(ncclUniqueId), all.data());
            if (g->IsMember() && g->Size() > 1) {
                ncclUniqueId gid = all[static_cast<size_t>(g->WorldRank(0))];
                NCCL_CHECK(ncclCommInitRank(&gc.prio_comm, g->Size(), gid,
                                            g->MyIdx()));
                int lo = 0, hi = 0;
                HIP_CHECKD(hipDeviceGetStreamPriorityRange(&lo, &hi));
                HIP_CHECKD(hipStreamCreateWithPriority(&gc.prio_stream,
                                                       hipStreamNonBlocking, hi));
            }
        }
        group_comms_.emplace(g->Uid(), std::move(gc));
        MLSL_LOG(DEBUG, "device comms ready for group uid=%d size=%d channels=%zu",
                 g->Uid(), g->Size(), nch);
    }

    GroupComms& For(ProcessGroup* g) {
        auto it = group_comms_.find(g->Uid());
        if (it == group_comms_.end()) {
            // Single-rank / self groups need no communicators; requests on
            // them take the local-copy path.
            MLSL_CHECK(g->Size() <= 1, "multi-rank group has no device comms");
            it = group_comms_.emplace(g->Uid(), GroupComms{}).first;
        }
        return it->second;
    }

  private:
    int device_id_;
    hipStream_t compute_stream_ = nullptr;  // null = legacy default stream
    std::unique_ptr<DevicePool> pool_;
    std::unordered_map<int, GroupComms> group_comms_;
    bool transport_decided_ = false;
    bool use_p2p_ = false;
};

}  // namespace

DeviceRuntime* CreateDeviceRuntime() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return nullptr;
    int local_rank = 0;
    if (const char* e = std::getenv("MLSL_LOCAL_RANK")) local_rank = std::atoi(e);
    else if (const char* e2 = std::getenv("LOCAL_RANK")) local_rank = std::atoi(e2);
    else local_rank = Bootstrap::EnvRank();
    auto* rt = new HipRuntime(local_rank % n);
    g_runtime = rt;
    return rt;
}

void DeviceSetupRequest(CommRequest* req, DeviceReqState& st) {
    // Persistent scratch only where the device executor needs it: the
    // compressed path (wire + residual), the custom schedule path (segment
    // staging), and the barrier token. The fused RCCL path allocates
    // nothing — one-shot hot-loop requests must not pay a hipMalloc+memset
    // per iteration.
    size_t tmp = 0;
    if (req->Compressed()) {
        // The dlopen'd compression plugin is a host-CPU contract
        // (reference ran it inside ep_server processes); silently running
        // the built-in kernels instead would not honor the user's library.
        MLSL_CHECK(req->Plugin() == nullptr,
                   "quantization plugin (lib_path) is supported on the host "
                   "transport only; device mode uses the built-in CDNA4 "
                   "kernels (unset lib_path)");
        for (auto& ce : req->Chunks()) tmp += ce.qplan.bytes;
    } else if (req->UsesDeviceSchedule()) {
        for (auto& ce : req->Chunks()) tmp += ce.sch.tmp_bytes;
    }
    if (req->Spec().op == CollOp::BARRIER) tmp = std::max<size_t>(tmp, 16);
    st.tmp_bytes = tmp;
    if (tmp) {
        st.tmp_dev = Context::Get().Device()->AllocDevice(tmp);
        // zero once: error-feedback residuals must start clean
        HIP_CHECKD(hipMemset(st.tmp_dev, 0, tmp));
    }
    if (req->Segmented()) {
        const std::vector<uint64_t>& offs = req->SegOffs();
        const size_t nseg = offs.size() - 1;
        st.seg_dev = Context::Get().Device()->AllocDevice(offs.size() * sizeof(uint64_t) +
                                                          nseg * sizeof(void*));
        HIP_CHECKD(hipMemcpy(st.seg_dev, offs.data(), offs.size() * sizeof(uint64_t),
                             hipMemcpyHostToDevice));
        void* pin = nullptr;
        HIP_CHECKD(hipHostMalloc(&pin, nseg * sizeof(void*)));
        st.seg_ptrs_pin = static_cast<void**>(pin);
    }
}

namespace {

enum class BufClass { DEV, PINNED, PAGEABLE };

BufClass ClassifyPtr(const void* p) {
    if (!p) return BufClass::DEV;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();
        return BufClass::PAGEABLE;  // unregistered host memory
    }
    if (attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged)
        return BufClass::DEV;
    if (attr.type == hipMemoryTypeHost || attr.type == hipMemoryTypeUnified)
        return BufClass::PINNED;    // registered host: DMA-able directly
    return BufClass::PAGEABLE;
}

// user<->pinned staging memcpy, multi-threaded above the configured
// threshold (reference MLSL_USE_COPY_THREADS, src/comm_ep.cpp:357-361,
// 1561-1574: OMP-threaded ReplaceIn copies; here plain std::thread ranges).
void HostStageCopy(void* dst, const void* src, size_t n) {
    const Config& cfg = GlobalConfig();
    if (n < cfg.copy_threshold || cfg.copy_threads <= 1) {
        std::memcpy(dst, src, n);
        return;
    }
    const size_t t = cfg.copy_threads;
    std::vector<std::thread> ths;
    for (size_t i = 0; i < t; ++i) {
        const size_t lo = i * n / t, hi = (i + 1) * n / t;
        ths.emplace_back([=]() {
            std::memcpy(static_cast<uint8_t*>(dst) + lo,
                        static_cast<const uint8_t*>(src) + lo, hi - lo);
        });
    }
    for (auto& th : ths) th.join();
}

// Bytes this rank contributes / receives for the whole request.
void IoBytes(CommRequest* req, size_t* send_b, size_t* recv_b) {
    const OpSpec& spec = req->Spec();
    const size_t es = DtypeSize(req->Dtype());
    const size_t N = static_cast<size_t>(req->Group()->Size());
    const bool is_root = req->Group()->MyIdx() == spec.root;
    size_t s = 0, r = 0;
    switch (spec.op) {
        case CollOp::ALLREDUCE: case CollOp::BCAST: case CollOp::REDUCE:
            s = r = spec.count * es;
            if (spec.op == CollOp::REDUCE && !is_root) r = spec.count * es; // scratch ok
            break;
        case CollOp::REDUCE_SCATTER: s = N * spec.count * es; r = spec.count * es; break;
        case CollOp::ALLGATHER: s = spec.count * es; r = N * spec.count * es; break;
        case CollOp::ALLGATHERV: {
            size_t t = 0;
            for (size_t c : spec.recv_counts) t += c;
            s = spec.recv_counts[req->Group()->MyIdx()] * es;
            r = t * es;
            break;
        }
        case CollOp::GATHER: s = spec.count * es; r = is_root ? N * spec.count * es : 0; break;
        case CollOp::SCATTER: s = is_root ? N * spec.count * es : 0; r = spec.count * es; break;
        case CollOp::ALLTOALL: s = r = N * spec.count * es; break;
        case CollOp::ALLTOALLV: {
            size_t ts = 0, tr = 0;
            for (size_t i = 0; i < N; ++i) {
                ts = std::max(ts, (spec.send_offs[i] + spec.send_counts[i]) * es);
                tr = std::max(tr, (spec.recv_offs[i] + spec.recv_counts[i]) * es);
            }
            s = ts; r = tr;
            break;
        }
        case CollOp::SRLIST: {
            size_t ts = 0, tr = 0;
            for (const auto& ppp : spec.pairs) {
                ts = std::max(ts, (ppp.send_off + ppp.send_count) * es);
                tr = std::max(tr, (ppp.recv_off + ppp.recv_count) * es);
            }
            s = ts; r = tr;
            break;
        }
        case CollOp::BARRIER: break;
    }
    *send_b = s;
    *recv_b = r;
}

// Whether the request's finish reads the recv buffer as well as writing it.
bool RecvIsInput(CommRequest* req) {
    if (!req->Compressed()) return false;
    for (const auto& ce : req->Chunks())
        if (ce.qplan.finish == QuantFinish::SCATTER && ce.qplan.accumulate) return true;
    return false;
}

// Issue one chunk through the fused RCCL op set.
void IssueFused(CommRequest* req, ChunkExec& ce, ncclComm_t comm, hipStream_t s,
                DeviceReqState& st) {
    const OpSpec& spec = req->Spec();
    ProcessGroup* g = req->Group();
    const size_t es = DtypeSize(req->Dtype());
    const uint8_t* sbase = req->SendBuf() + ce.elem_off * es;
    uint8_t* rbase = req->RecvBuf() + ce.elem_off * es;
    const size_t cnt = [&]() -> size_t {
        // chunk-local element count for splittable ops
        switch (spec.op) {
            case CollOp::ALLREDUCE:
            case CollOp::BCAST:
            case CollOp::REDUCE: {
                // Recover from the schedule result size.
                return ce.sch.result.bytes / es;
            }
            default:
                return spec.count;
        }
    }();
    const ncclDataType_t ndt = ToNccl(req->Dtype());
    const ncclRedOp_t nop = ToNcclOp(spec.rop);
    const int gsize = g->Size();

    switch (spec.op) {
        case CollOp::ALLREDUCE:
            NCCL_CHECK(ncclAllReduce(sbase, rbase, cnt, ndt, nop, comm, s));
            break;
        case CollOp::REDUCE:
            NCCL_CHECK(ncclReduce(sbase, rbase, cnt, ndt, nop, spec.root, comm, s));
            break;
        case CollOp::BCAST:
            NCCL_CHECK(ncclBroadcast(rbase, rbase, cnt, ndt, spec.root, comm, s));
            break;
        case CollOp::REDUCE_SCATTER:
            NCCL_CHECK(ncclReduceScatter(sbase, rbase, spec.count, ndt, nop, comm, s));
            break;
        case CollOp::ALLGATHER:
            NCCL_CHECK(ncclAllGather(sbase, rbase, spec.count, ndt, comm, s));
            break;
        case CollOp::ALLGATHERV: {
            // grouped bcast-equivalent: every rank sends its block to all.
            std::vector<size_t> offs(gsize + 1, 0);
            for (int i = 0; i < gsize; ++i) offs[i + 1] = offs[i] + spec.recv_counts[i] * es;
            NCCL_CHECK(ncclGroupStart());
            for (int i = 0; i < gsize; ++i) {
                if (i == g->MyIdx()) continue;
                NCCL_CHECK(ncclSend(sbase, spec.recv_counts[g->MyIdx()], ndt, i, comm, s));
                NCCL_CHECK(ncclRecv(rbase + offs[i], spec.recv_counts[i], ndt, i, comm, s));
            }
            NCCL_CHECK(ncclGroupEnd());
            LaunchCopy(rbase + offs[g->MyIdx()], sbase,
                       spec.recv_counts[g->MyIdx()] * es, s);
            break;
        }
        case CollOp::GATHER: {
            NCCL_CHECK(ncclGroupStart());
            if (g->MyIdx() == spec.root) {
                for (int i = 0; i < gsize; ++i) {
                    if (i == spec.root) continue;
                    NCCL_CHECK(ncclRecv(rbase + i * spec.count * es, spec.count, ndt, i, comm, s));
                }
            } else {
                NCCL_CHECK(ncclSend(sbase, spec.count, ndt, spec.root, comm, s));
            }
            NCCL_CHECK(ncclGroupEnd());
            if (g->MyIdx() == spec.root)
                LaunchCopy(rbase + spec.root * spec.count * es, sbase,
                           spec.count * es, s);
            break;
        }
        case CollOp::SCATTER: {
            NCCL_CHECK(ncclGroupStart());
            if (g->MyIdx() == spec.root) {
                for (int i = 0; i < gsize; ++i) {
                    if (i == spec.root) continue;
                    NCCL_CHECK(ncclSend(sbase + i * spec.count * es, spec.count, ndt, i, comm, s));
                }
            } else {
                NCCL_CHECK(ncclRecv(rbase, spec.count, ndt, spec.root, comm, s));
            }
            NCCL_CHECK(ncclGroupEnd());
            if (g->MyIdx() == spec.root)
                LaunchCopy(rbase, sbase + spec.root * spec.count * es,
                           spec.count * es, s);
            break;
        }
        case CollOp::ALLTOALL: {
            NCCL_CHECK(ncclGroupStart());
            for (int i = 0; i < gsize; ++i) {
                if (i == g->MyIdx()) continue;
                NCCL_CHECK(ncclSend(sbase + i * spec.count * es, spec.count, ndt, i, comm, s));
                NCCL_CHECK(ncclRecv(rbase + i * spec.count * es, spec.count, ndt, i, comm, s));
            }
            NCCL_CHECK(ncclGroupEnd());
            LaunchCopy(rbase + g->MyIdx() * spec.count * es,
                       sbase + g->MyIdx() * spec.count * es, spec.count * es, s);
            break;
        }
        case CollOp::ALLTOALLV: {
            NCCL_CHECK(ncclGroupStart());
            for (int i = 0; i < gsize; ++i) {
                if (i == g->MyIdx()) continue;
                NCCL_CHECK(ncclSend(sbase + spec.send_offs[i] * es, spec.send_counts[i], ndt, i, comm, s));
                NCCL_CHECK(ncclRecv(rbase + spec.recv_offs[i] * es, spec.recv_counts[i], ndt, i, comm, s));
            }
            NCCL_CHECK(ncclGroupEnd());
            LaunchCopy(rbase + spec.recv_offs[g->MyIdx()] * es,
                       sbase + spec.send_offs[g->MyIdx()] * es,
                       spec.send_counts[g->MyIdx()] * es, s);
            break;
        }
        case CollOp::BARRIER:
            NCCL_CHECK(ncclAllReduce(st.tmp_dev, st.tmp_dev, 1, ncclFloat32, ncclSum, comm, s));
            break;
        case CollOp::SRLIST: {
            NCCL_CHECK(ncclGroupStart());
            for (const auto& p : spec.pairs) {
                if (p.send_count)
                    NCCL_CHECK(ncclSend(sbase + p.send_off * es, p.send_count, ndt, p.peer, comm, s));
                if (p.recv_count)
                    NCCL_CHECK(ncclRecv(rbase + p.recv_off * es, p.recv_count, ndt, p.peer, comm, s));
            }
            NCCL_CHECK(ncclGroupEnd());
            break;
        }
    }
}

// Issue one chunk by walking its schedule: per phase a grouped
// ncclSend/ncclRecv, then the local reduce kernel / async copy. This is the
// hand-written collective path (ring/RHD over explicit p2p) — RCCL supplies
// transport, OUR schedule supplies the algorithm and OUR kernels the math.
void IssueSchedule(CommRequest* req, ChunkExec& ce, ncclComm_t comm, hipStream_t s,
                   const uint8_t* sbase, uint8_t* rbase, uint8_t* tmp_dev) {
    const ncclDataType_t ndt = ncclUint8;  // byte-addressed transfers
    auto ptr = [&](const BufRef& b) { return SpacePtr(b, sbase, rbase, tmp_dev); };

    for (int phase = 0; phase < ce.sch.num_phases; ++phase) {
        bool grouped = false;
        for (const auto& st : ce.sch.steps) {
            if (st.phase != phase) continue;
            if ((st.send_peer >= 0 && st.send.bytes) || (st.recv_peer >= 0 && st.recv.bytes)) {
                if (!grouped) {
                    NCCL_CHECK(ncclGroupStart());
                    grouped = true;
                }
                if (st.send_peer >= 0 && st.send.bytes)
                    NCCL_CHECK(ncclSend(ptr(st.send), st.send.bytes, ndt, st.send_peer, comm, s));
                if (st.recv_peer >= 0 && st.recv.bytes)
                    NCCL_CHECK(ncclRecv(ptr(st.recv), st.recv.bytes, ndt, st.recv_peer, comm, s));
            }
        }
        if (grouped) NCCL_CHECK(ncclGroupEnd());
        for (const auto& st : ce.sch.steps) {
            if (st.phase != phase || st.local == Step::LocalOp::NONE) continue;
            if (st.local_dst.bytes == 0) continue;  // zero-length segment
            // a compressed chunk's sbase is its plan's base (IssueAll)
            LaunchLocalOp(st, ptr(st.local_dst), ptr(st.local_src), ce.qplan,
                          const_cast<uint8_t*>(sbase), req->Dtype(), ce.sch.rop,
                          req->QParams().WireBlockBytes(), s, /*nt=*/true);
        }
    }
}

// One compressed chunk whose plan regions (quant_plan.hpp) start at `base`:
// quantize every send segment where the plan says, residual alongside if it
// has one; let `walk(wire, scratch)`
// run the schedule over the wire; finish into rbuf. `walk` is the only thing
// the executors differ in: nothing at n=1, the IPC window walker, or the
// RCCL one.
// An allreduce over a tensor list (one plan segment, a DEQUANT finish) has no
// sbuf or rbuf: its prologue and finish go through the tables in `st`. A
// reduce-scatter over a tensor list has no sbuf: only its prologue does, and
// the flat reduce-scatter's finish writes rbuf.
template <class Walk>
void IssueCompressed(CommRequest* req, const DeviceReqState& st, const ChunkExec& ce,
                     uint8_t* base, const uint8_t* sbuf, uint8_t* rbuf, hipStream_t s,
                     Walk&& walk) {
    const QuantPlan& p = ce.qplan;
    const DataType dt = req->Dtype();
    const bool seg = req->Segmented();
    const bool seg_rs = req->SegmentedReduceScatter();
    const size_t nseg = seg ? req->SegPtrs().size() : 0;
    const uint64_t* seg_offs = static_cast<const uint64_t*>(st.seg_dev);
    void** seg_ptrs = seg ? reinterpret_cast<void**>(
                                static_cast<uint8_t*>(st.seg_dev) + (nseg + 1) * sizeof(uint64_t))
                          : nullptr;
    if (seg) {
        // this start's pointers, pinned host to device on the request's
        // stream; the last start was waited for, so the mirror is free
        std::memcpy(st.seg_ptrs_pin, req->SegPtrs().data(), nseg * sizeof(void*));
        HIP_CHECKD(hipMemcpyAsync(seg_ptrs, st.seg_ptrs_pin, nseg * sizeof(void*),
                                  hipMemcpyHostToDevice, s));
        if (seg_rs)
            // all N shards of the padded concatenation in one launch
            LaunchQuantizeGatherShards(seg_ptrs, seg_offs, nseg,
                                       p.residual ? base + p.err_off : nullptr,
                                       base + p.send_seg * p.seg_wire,
                                       static_cast<size_t>(req->SegOffs().back()), p.nseg,
                                       p.count, p.seg_wire, p.block, dt, p.residual, s);
        else
            LaunchQuantizeGather(seg_ptrs, seg_offs, nseg,
                                 p.residual ? base + p.err_off : nullptr,
                                 base + p.send_seg * p.seg_wire, p.count, p.block, dt,
                                 p.residual, s);
    } else {
        for (size_t j = 0; j < p.nseg; ++j)
            LaunchQuantize(sbuf + j * p.seg_bytes,
                           p.residual ? base + p.err_off + j * p.seg_bytes : nullptr,
                           base + (p.send_seg + j) * p.seg_wire, p.count, p.block, dt,
                           p.residual, s);
    }
    walk(base, base + p.scratch_off);
    const void* wires[kQuantRsDirectMaxRanks];
    FinishWires(p, base, wires);
    switch (p.finish) {
        case QuantFinish::SUMN:
            LaunchQuantSumDequantN(wires, p.nwires, rbuf, p.count, p.block, dt, s);
            break;
        case QuantFinish::SUM2:
            LaunchQuantSumDequant(wires[0], wires[1], rbuf, p.count, p.block, dt, s);
            break;
        case QuantFinish::DEQUANT:
            if (seg && !seg_rs)
                // round_first: the flat request's bits, then scaled
                LaunchDequantizeScatter(wires[0], seg_ptrs, seg_offs, nseg, p.count, p.block,
                                        dt, req->PostScale(), /*round_first=*/true, s);
            else
                LaunchDequantize(wires[0], rbuf, p.count, p.block, dt, s);
            break;
        case QuantFinish::SCATTER:
            LaunchDequantizeSegments(wires[0], p.out_segs, rbuf, p.count, p.block, dt,
                                     p.accumulate, s);
            break;
    }
}

bool GraphEligible(CommRequest* req, GroupComms& gc) {
    // Single effective stream only: every chunk must land on channel 0 and
    // no host staging (H2D/D2H of *pageable* memory is not capturable).
    // a tensor list's pointers change from start to start and reach the device
    // by a copy from a host mirror written at issue: nothing to replay
    if (req->Segmented()) return false;
    if (req->Compressed()) return true;  // single stream by construction
    if (gc.comms.size() > 1 && req->Chunks().size() > 1) return false;
    return true;
}

bool AllEventsDone(DeviceReqState& st) {
    for (hipEvent_t e : st.events) {
        hipError_t q = hipEventQuery(e);
        if (q == hipErrorNotReady) return false;
        if (q != hipSuccess) MLSL_THROW(std::string("HIP event error: ") +
                                        hipGetErrorString(q));
    }
    return true;
}

void EnsureEvents(DeviceReqState& st, size_t n) {
    // Timing-capable events when MLSL_STATS is on (hipEvent-backed device
    // statistics); the cheaper no-timestamp flavor otherwise.
    const unsigned flags =
        GlobalConfig().stats ? hipEventDefault : hipEventDisableTiming;
    while (st.events.size() < n) {
        hipEvent_t e;
        HIP_CHECKD(hipEventCreateWithFlags(&e, flags));
        st.events.push_back(e);
    }
}

// Completion check + the deferred pinned->user unstage memcpy (pageable
// recv buffers: the D2H leg landed in the pinned bounce on-stream; the
// final host copy runs once, here, after the events fire).
bool DeviceFinishIfDone(CommRequest* req, DeviceReqState& st) {
    if (!AllEventsDone(st)) return false;
    if (st.unstage_pending) {
        HostStageCopy(req->UserRecvBuf(), st.pin_recv, st.unstage_bytes);
        st.unstage_pending = false;
    }
    return true;
}

// Record st.dep_event (created on first use) on `src`.
void RecordDep(DeviceReqState& st, hipStream_t src) {
    if (!st.dep_event)
        HIP_CHECKD(hipEventCreateWithFlags(&st.dep_event, hipEventDisableTiming));
    HIP_CHECKD(hipEventRecord(st.dep_event, src));
}

// The other channel streams order after what stream 0 carries so far.
void FanOutStream0(GroupComms& gc, DeviceReqState& st) {
    if (gc.streams.size() <= 1) return;
    RecordDep(st, gc.streams[0]);
    for (size_t i = 1; i < gc.streams.size(); ++i)
        HIP_CHECKD(hipStreamWaitEvent(gc.streams[i], st.dep_event, 0));
}

// Grow a persistent HBM (or pinned host) buffer to at least `need` bytes.
void GrowBuffer(HipRuntime* rt, void*& buf, size_t& have, size_t need, bool pinned) {
    if (buf && have >= need) return;
    if (pinned) {
        if (buf) (void)hipHostFree(buf);
        HIP_CHECKD(hipHostMalloc(&buf, need));
    } else {
        if (buf) rt->FreeDevice(buf);
        buf = rt->AllocDevice(need);
    }
    have = need;
}

// Stage the result out: D2H into the pinned bounce (pageable user memory) or
// straight into the user's registered buffer.
void EnqueueUnstage(CommRequest* req, DeviceReqState& st, hipStream_t s) {
    HIP_CHECKD(hipMemcpyAsync(
        st.unstage_pending ? st.pin_recv : static_cast<void*>(req->UserRecvBuf()),
        st.stage_recv, st.unstage_bytes, hipMemcpyDeviceToHost, s));
}

// Order after the caller's compute stream: the producer kernels
// (e.g. torch backward on the default stream) must land before the
// collective reads the buffers. When the compute stream is idle
// (hipStreamQuery ~0.1 us) there is nothing to order against and
// the record+wait pair (~4.5 us on the legacy stream) is skipped.
void OrderAfterCompute(HipRuntime* rt, GroupComms& gc, DeviceReqState& st) {
    hipStream_t comp = static_cast<hipStream_t>(rt->ComputeStream());
    hipError_t q = hipStreamQuery(comp);
    if (q != hipSuccess) {
        (void)hipGetLastError();
        RecordDep(st, comp);
        for (hipStream_t cs : gc.streams)
            HIP_CHECKD(hipStreamWaitEvent(cs, st.dep_event, 0));
    }
}

// hipGraph replay (MLSL_USE_GRAPHS): same request + same buffers ->
// launch the captured graph instead of re-enqueueing.
bool ReplayGraph(CommRequest* req, GroupComms& gc, DeviceReqState& st) {
    if (!st.graph_exec || req->SendBuf() != st.captured_sbuf ||
        req->RecvBuf() != st.captured_rbuf)
        return false;
    HIP_CHECKD(hipGraphLaunch(st.graph_exec, gc.streams[0]));
    EnsureEvents(st, 1);
    HIP_CHECKD(hipEventRecord(st.events[0], gc.streams[0]));
    st.issued = true;
    return true;
}

// Host-buffer staging (ReplaceIn analog): stage host buffers through
// persistent HBM so RCCL/kernels see device memory. Pageable memory
// bounces through a persistent PINNED buffer in chunks — the H2D DMA of
// chunk k overlaps the host memcpy of chunk k+1; already-pinned user
// buffers DMA directly. (Classified fresh every Start:
// hipPointerGetAttributes is ~0.3 us and a pointer-value cache would
// misclassify a freed-and-reallocated pointer.) Returns whether either
// buffer was staged.
bool StageIn(CommRequest* req, HipRuntime* rt, GroupComms& gc, DeviceReqState& st,
               hipStream_t base_s) {
    size_t send_b = 0, recv_b = 0;
    IoBytes(req, &send_b, &recv_b);
    const BufClass s_cls = send_b > 0 ? ClassifyPtr(req->UserSendBuf())
                                      : BufClass::DEV;
    const BufClass r_cls = recv_b > 0 ? ClassifyPtr(req->UserRecvBuf())
                                      : BufClass::DEV;
    const bool s_host = s_cls != BufClass::DEV;
    const bool r_host = r_cls != BufClass::DEV;
    st.recv_staged = r_host;
    st.unstage_pending = false;
    constexpr size_t kStageChunk = 32u << 20;
    if (s_host) {
        GrowBuffer(rt, st.stage_send, st.stage_send_bytes, send_b, false);
        if (s_cls == BufClass::PINNED) {
            HIP_CHECKD(hipMemcpyAsync(st.stage_send, req->UserSendBuf(), send_b,
                                      hipMemcpyHostToDevice, base_s));
        } else {
            GrowBuffer(rt, st.pin_send, st.pin_send_bytes, send_b, true);
            for (size_t off = 0; off < send_b; off += kStageChunk) {
                const size_t n = std::min(kStageChunk, send_b - off);
                HostStageCopy(static_cast<uint8_t*>(st.pin_send) + off,
                              req->UserSendBuf() + off, n);
                HIP_CHECKD(hipMemcpyAsync(
                    static_cast<uint8_t*>(st.stage_send) + off,
                    static_cast<uint8_t*>(st.pin_send) + off, n,
                    hipMemcpyHostToDevice, base_s));
            }
        }
        FanOutStream0(gc, st);
    }
    if (r_host) {
        GrowBuffer(rt, st.stage_recv, st.stage_recv_bytes, recv_b, false);
        if (r_cls == BufClass::PAGEABLE)
            GrowBuffer(rt, st.pin_recv, st.pin_recv_bytes, recv_b, true);
        // Pageable: D2H lands in the pinned bounce; the final pinned->user
        // memcpy runs host-side once the completion events fire.
        st.unstage_pending = r_cls == BufClass::PAGEABLE;
        st.unstage_bytes = recv_b;
        // BCAST is an in-place op: its schedule reads the payload from
        // RECV space (no SEND-space step), so the staged input must land
        // in stage_recv as well — without this the staged root broadcasts
        // an uninitialized buffer (caught by the e2e param-consistency
        // check on the device engine).
        if (req->Spec().op == CollOp::BCAST && s_host) {
            LaunchCopy(st.stage_recv, st.stage_send, recv_b, base_s);
            // re-fan-out: channel streams must order after this copy
            // too, not only after the send staging
            FanOutStream0(gc, st);
        }
        // An accumulating finish (quantized all-gather) READS recv: the
        // user's values have to be in stage_recv before it runs. Pinned
        // memory DMAs directly; pageable memory bounces through pin_recv in
        // chunks as the send side does (the D2H of the result lands there
        // only after everything issued below).
        if (RecvIsInput(req)) {
            if (r_cls == BufClass::PINNED) {
                HIP_CHECKD(hipMemcpyAsync(st.stage_recv, req->UserRecvBuf(), recv_b,
                                          hipMemcpyHostToDevice, base_s));
            } else {
                for (size_t off = 0; off < recv_b; off += kStageChunk) {
                    const size_t n = std::min(kStageChunk, recv_b - off);
                    HostStageCopy(static_cast<uint8_t*>(st.pin_recv) + off,
                                  req->UserRecvBuf() + off, n);
                    HIP_CHECKD(hipMemcpyAsync(
                        static_cast<uint8_t*>(st.stage_recv) + off,
                        static_cast<uint8_t*>(st.pin_recv) + off, n,
                        hipMemcpyHostToDevice, base_s));
                }
            }
            FanOutStream0(gc, st);
        }
    }
    req->SetDeviceBuffers(s_host ? static_cast<const uint8_t*>(st.stage_send) : nullptr,
                          r_host ? static_cast<uint8_t*>(st.stage_recv) : nullptr);
    return s_host || r_host;
}

// Order the priority lane after the producers and any staging H2D:
// both dependencies are carried by channel stream 0 at this point
// (it waited on the compute stream above if that was busy, and the
// staging copy was enqueued on it), so record a fresh event there
// unconditionally — st.dep_event may not exist yet when the compute
// stream was idle and no staging ran.
void OrderPriorityLane(GroupComms& gc, DeviceReqState& st) {
    RecordDep(st, gc.streams[0]);
    HIP_CHECKD(hipStreamWaitEvent(gc.prio_stream, st.dep_event, 0));
}

// What one Start decided before it issues.
struct IssueCtx {
    hipStream_t base_s = nullptr;  // n=1: the compute stream (short) or stream 0
    bool prio = false;             // everything rides the priority lane
    bool p2p = false;              // IPC window transport
    size_t nch = 1;                // channels chunks are dealt over
};

void IssueAll(CommRequest* req, GroupComms& gc, DeviceReqState& st, const IssueCtx& ic) {
    auto& chunks = req->Chunks();
    const size_t es = DtypeSize(req->Dtype());
    const bool compressed = req->Compressed();
    const bool use_schedule = req->UsesDeviceSchedule();
    if (gc.comms.empty() && !ic.p2p) {
        hipStream_t s0 = ic.base_s;
        for (auto& ce : chunks) {
            const uint8_t* sbase = req->SendBuf() + ce.elem_off * es;
            uint8_t* rbase = req->RecvBuf() + ce.elem_off * es;
            if (compressed) {
                // quantize -> dequantize keeps the quantized
                // collective's semantics (and error feedback) at n=1
                IssueCompressed(req, st, ce, static_cast<uint8_t*>(st.tmp_dev), sbase, rbase,
                                s0, [](uint8_t*, uint8_t*) {});
            } else if (ce.sch.result.bytes && sbase != rbase) {
                // NT copy kernel: measured faster than the blit path for
                // large streams (docs/BENCHMARKS.md); buffers are device
                // memory here (host users are staged above).
                LaunchCopy(rbase + ce.sch.result.off, sbase,
                           ce.sch.result.bytes, s0);
            }
        }
        if (st.recv_staged) EnqueueUnstage(req, st, s0);
        return;
    }
    size_t tmp_off = 0;
    for (auto& ce : chunks) {
        const size_t ch = ce.chunk_idx % ic.nch;
        hipStream_t strm_ = ic.prio ? gc.prio_stream : gc.streams[ch];
        uint8_t* tbase = static_cast<uint8_t*>(st.tmp_dev) + tmp_off;
        // IPC window transport: every op walks its schedule; lane
        // nlanes-1 is the priority lane.
        const size_t lane = !ic.p2p ? 0 : ic.prio ? gc.p2p->Lanes() - 1 : ch;
        ncclComm_t comm_ = ic.p2p ? nullptr : ic.prio ? gc.prio_comm : gc.comms[ch];
        auto walk = [&](const uint8_t* sbase, uint8_t* rbase, uint8_t* scratch) {
            if (ic.p2p)
                gc.p2p->IssueSchedule(req->Dtype(), req->QParams().WireBlockBytes(), ce, lane,
                                      strm_, sbase, rbase, scratch);
            else IssueSchedule(req, ce, comm_, strm_, sbase, rbase, scratch);
        };
        if (compressed) {
            // quantize -> compressed-domain ring -> dequantize (driver
            // config 5: int8 allreduce / reduce-scatter of bf16/f32 grads)
            IssueCompressed(req, st, ce, tbase, req->SendBuf(), req->RecvBuf(), strm_,
                            [&](uint8_t* wire, uint8_t* scratch) { walk(wire, wire, scratch); });
            tmp_off += ce.qplan.bytes;
        } else if (ic.p2p || use_schedule) {
            walk(req->SendBuf() + ce.elem_off * es, req->RecvBuf() + ce.elem_off * es, tbase);
            tmp_off += ce.sch.tmp_bytes;
        } else {
            IssueFused(req, ce, comm_, strm_, st);
            tmp_off += ce.sch.tmp_bytes;
        }
    }
}

// Issue eagerly, or (try_capture) capture the issue into a hipGraph, launch
// it and keep it for replay; a capture that fails at either end falls back
// to eager for good.
void IssueOrCapture(CommRequest* req, GroupComms& gc, DeviceReqState& st,
                    const IssueCtx& ic, bool try_capture) {
    if (!try_capture) {
        IssueAll(req, gc, st, ic);
        return;
    }
    bool body_ok = true;
    hipError_t ce0 = hipStreamBeginCapture(gc.streams[0],
                                           hipStreamCaptureModeThreadLocal);
    if (ce0 == hipSuccess) {
        try {
            IssueAll(req, gc, st, ic);
        } catch (const std::exception&) {
            body_ok = false;
        }
        hipGraph_t graph = nullptr;
        hipError_t ce1 = hipStreamEndCapture(gc.streams[0], &graph);
        if (body_ok && ce1 == hipSuccess && graph &&
            hipGraphInstantiate(&st.graph_exec, graph, nullptr, nullptr, 0) ==
                hipSuccess) {
            (void)hipGraphDestroy(graph);
            st.captured_sbuf = req->SendBuf();
            st.captured_rbuf = req->RecvBuf();
            HIP_CHECKD(hipGraphLaunch(st.graph_exec, gc.streams[0]));
        } else {
            // capture produced nothing executable -> run eagerly
            (void)hipGetLastError();
            if (graph) (void)hipGraphDestroy(graph);
            st.graph_exec = nullptr;
            st.graph_failed = true;
            IssueAll(req, gc, st, ic);
        }
    } else {
        (void)hipGetLastError();
        st.graph_failed = true;
        IssueAll(req, gc, st, ic);
    }
}

// Completion events (outside any graph). Graph path + single-channel
// path complete on stream 0; multi-channel records one per channel.
void RecordCompletion(CommRequest* req, GroupComms& gc, DeviceReqState& st,
                      const IssueCtx& ic) {
    if (st.graph_exec || (gc.comms.empty() && !ic.p2p)) {
        EnsureEvents(st, 1);
        HIP_CHECKD(hipEventRecord(st.events[0],
                                  st.graph_exec ? gc.streams[0] : ic.base_s));
        return;
    }
    const size_t used = std::min(req->Chunks().size(), ic.nch);
    EnsureEvents(st, used);
    for (size_t ch = 0; ch < used; ++ch)
        HIP_CHECKD(hipEventRecord(st.events[ch],
                                  ic.prio ? gc.prio_stream : gc.streams[ch]));
    if (st.recv_staged) {
        // join all channels on stream 0, then stage the result out
        for (size_t ch = 0; ch < used; ++ch)
            HIP_CHECKD(hipStreamWaitEvent(gc.streams[0], st.events[ch], 0));
        EnqueueUnstage(req, st, gc.streams[0]);
        EnsureEvents(st, used + 1);
        HIP_CHECKD(hipEventRecord(st.events[used], gc.streams[0]));
    }
}

}  // namespace

void DeviceCheckSegmentPointers(void* const* ptrs, size_t nseg) {
    for (size_t j = 0; j < nseg; ++j)
        MLSL_CHECK(ClassifyPtr(ptrs[j]) == BufClass::DEV,
                   "start over a tensor list: tensor " + std::to_string(j) +
                       " is not device memory (no staging is built for this request; "
                       "move it to the device)");
}

bool DeviceIsDevicePointer(const void* p) { return ClassifyPtr(p) == BufClass::DEV; }

double DeviceRequestCommMs(DeviceReqState& st) {
    if (!st.timed || !st.t0_event || st.events.empty()) return -1.0;
    float best = -1.0f;
    for (hipEvent_t e : st.events) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, st.t0_event, e) == hipSuccess) {
            if (ms > best) best = ms;
        } else {
            (void)hipGetLastError();
        }
    }
    return best;
}

bool DeviceAdvanceRequest(CommRequest* req, DeviceReqState& st) {
    auto* rt = static_cast<HipRuntime*>(Context::Get().Device());
    GroupComms& gc = rt->For(req->Group());
    if (st.issued) {
        // Wait kernels abort (host word / wall-clock bound) instead of
        // wedging the GPU; surface that as a loud request failure.
        if (gc.p2p && !gc.p2p->Healthy())
            MLSL_THROW("p2p transport wait aborted (peer dead or timeout)");
        return DeviceFinishIfDone(req, st);
    }
    IssueCtx ic;
    ic.p2p = gc.p2p != nullptr;
    if (gc.comms.empty() && gc.streams.empty() && !ic.p2p) {
        hipStream_t s0;
        HIP_CHECKD(hipStreamCreateWithFlags(&s0, hipStreamNonBlocking));
        gc.streams.push_back(s0);
    }
    const Config& cfg = GlobalConfig();
    // Reference MLSL_MAX_SHORT_MSG_SIZE analog: small world-1 messages
    // issue directly on the compute stream — same-stream ordering makes
    // the dep-event handshake (two extra HIP calls of the small-message
    // floor) unnecessary. Large messages keep the side stream for overlap.
    const bool short_local = gc.comms.empty() && !ic.p2p &&
                             req->MessageBytes() <= cfg.max_short_msg;
    ic.base_s = short_local ? static_cast<hipStream_t>(rt->ComputeStream())
                            : gc.streams[0];
    if (!short_local) {
        OrderAfterCompute(rt, gc, st);
        if (ReplayGraph(req, gc, st)) return AllEventsDone(st);
    }

    const bool staged = StageIn(req, rt, gc, st, ic.base_s);
    ic.prio = cfg.msg_priority &&
              (gc.prio_comm || (ic.p2p && gc.prio_stream)) &&
              req->MessageBytes() >= cfg.msg_priority_threshold;
    if (ic.prio) OrderPriorityLane(gc, st);

    // Graph capture only when everything lands on ONE capturable stream:
    // no pageable staging, no priority lane, single channel.
    const bool try_capture = cfg.use_graphs && !st.graph_failed && !staged &&
                             !ic.prio && !short_local && !ic.p2p &&
                             GraphEligible(req, gc);

    // hipEvent device timing (MLSL_STATS): t0 on the stream that issues
    // first; completion events are timing-capable (EnsureEvents).
    st.timed = cfg.stats;
    if (st.timed) {
        if (!st.t0_event)
            HIP_CHECKD(hipEventCreateWithFlags(&st.t0_event, hipEventDefault));
        HIP_CHECKD(hipEventRecord(st.t0_event, ic.prio ? gc.prio_stream : ic.base_s));
    }

    ic.nch = ic.p2p ? std::max<size_t>(1, gc.streams.size())
                    : (gc.comms.empty() ? 1 : gc.comms.size());
    IssueOrCapture(req, gc, st, ic, try_capture);
    RecordCompletion(req, gc, st, ic);
    st.issued = true;
    return DeviceFinishIfDone(req, st);
}

}  // namespace mlsl
