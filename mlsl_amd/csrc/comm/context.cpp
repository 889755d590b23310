#include "context.hpp"

#include <unistd.h>

#include <cstdlib>
#include <cstring>

#include "../core/log.hpp"
#include "../core/signals.hpp"
#include "../core/sysinfo.hpp"
#include "../core/types.hpp"
#include "device_comm.hpp"
#include "request.hpp"

namespace mlsl {

static bool g_initialized = false;

Context& Context::Get() {
    static Context ctx;
    return ctx;
}

bool Context::Initialized() { return g_initialized; }

void Context::Init(int rank, int size) {
    MLSL_CHECK(!initialized_, "Context::Init called twice");
    Config& cfg = GlobalConfig();
    cfg = Config::FromEnv();  // re-read: tests mutate env between inits
    CheckQuantBlock(cfg.quant_block, "MLSL_QUANT_BLOCK");
    SetLogLevel(static_cast<LogLevel>(cfg.log_level));

    InstallSignalHandlers();
    AutoConfig();

    boot_ = std::make_unique<Bootstrap>(rank, size);
    boot_rank_ = boot_->Rank();
    boot_size_ = boot_->Size();
    rank_ = boot_rank_;
    size_ = boot_size_;

    // Transport selection: device mode when a HIP device is visible unless
    // MLSL_TRANSPORT forces tcp.
    device_mode_ = false;
    if (cfg.transport != "tcp") {
        device_.reset(CreateDeviceRuntime());
        if (device_) {
            device_mode_ = true;
            device_id_ = device_->DeviceId();
        } else if (cfg.transport == "rccl") {
            MLSL_THROW("MLSL_TRANSPORT=rccl but no HIP device is visible");
        }
    }

    if (size_ > 1) mesh_ = std::make_unique<Mesh>(*boot_);
    engine_ = std::make_unique<Engine>(mesh_.get(), cfg.progress, device_mode_);

    // World and self groups.
    {
        std::vector<int> all(static_cast<size_t>(boot_size_));
        for (int i = 0; i < boot_size_; ++i) all[i] = i;
        groups_.push_back(std::make_unique<ProcessGroup>(next_group_uid_++, all, boot_rank_));
        world_ = groups_.back().get();
        groups_.push_back(std::make_unique<ProcessGroup>(
            next_group_uid_++, std::vector<int>{boot_rank_}, boot_rank_));
        self_ = groups_.back().get();
    }
    if (device_mode_) device_->EnsureGroupComms(world_);

    initialized_ = true;
    init_pid_ = static_cast<long>(getpid());
    g_initialized = true;
    if (rank_ == 0) cfg.Dump();
    MLSL_LOG(INFO, "mlsl context up: rank %d/%d mode=%s", rank_, size_,
             device_mode_ ? device_->Name().c_str() : "host-tcp");
}

void Context::Finalize() {
    if (!initialized_) return;
    // Fork safety (reference src/mlsl.cpp:720-724): a forked child (e.g. a
    // data-loader worker, or an atexit handler in a fork+exec helper) must
    // not tear down the parent's sockets, progress thread, or HIP state —
    // Finalize is a no-op in any pid other than the one that called Init.
    if (static_cast<long>(getpid()) != init_pid_) {
        MLSL_LOG(DEBUG, "Finalize in forked child pid — skipping teardown");
        return;
    }
    // MPI_Finalize semantics: no rank closes its mesh sockets until every
    // rank has finished its last collective (ranks reach Finalize at
    // different times; without this, an early-closing rank makes the
    // peer's progress loop see EOF mid-teardown).
    if (boot_ && mesh_) {
        try {
            boot_->Barrier();
        } catch (const std::exception& e) {
            MLSL_LOG(ERROR, "finalize barrier failed (peer died?): %s", e.what());
        }
    }
    engine_.reset();      // join progress thread first
    groups_.clear();
    world_ = self_ = nullptr;
    mesh_.reset();
    boot_.reset();
    {
        std::lock_guard<std::mutex> lk(alloc_mu_);
        for (auto& kv : allocs_) {
            if (kv.second.device) {
                if (device_) device_->FreeDevice(const_cast<void*>(kv.first));
            } else {
                std::free(const_cast<void*>(kv.first));
            }
        }
        allocs_.clear();
    }
    device_.reset();
    next_group_uid_ = 0;
    initialized_ = false;
    g_initialized = false;
}

void Context::Configure(int tenant_color) {
    MLSL_CHECK(initialized_, "Context not initialized");
    tenant_color_ = tenant_color;
    // Re-split the world by tenant color; groups and Rank/Size become
    // tenant-relative (reference Configure color-split semantics).
    struct TC { int32_t tenant; int32_t color; };
    std::vector<TC> all(static_cast<size_t>(boot_size_));
    TC mine{tenant_color_, 0};
    boot_->Allgather(&mine, sizeof(TC), all.data());
    std::vector<int> members;
    for (int i = 0; i < boot_size_; ++i)
        if (all[i].tenant == tenant_color_) members.push_back(i);
    groups_.push_back(std::make_unique<ProcessGroup>(next_group_uid_++, members,
                                                     boot_rank_));
    world_ = groups_.back().get();
    rank_ = world_->MyIdx();
    size_ = world_->Size();
    if (device_mode_) device_->EnsureGroupComms(world_);
    MLSL_LOG(INFO, "configured tenant color=%d: rank %d/%d", tenant_color_, rank_,
             size_);
}

ProcessGroup* Context::CreateGroup(int color) {
    MLSL_CHECK(initialized_, "Context not initialized");
    // Collective color exchange over the bootstrap (MPI_Comm_split analog,
    // ordered by world rank — reference src/comm_ep.cpp:1821-1827).
    // Colors are namespaced by tenant so Configure'd sub-worlds cannot
    // accidentally merge groups.
    struct TC { int32_t tenant; int32_t color; };
    std::vector<TC> colors(static_cast<size_t>(boot_size_));
    TC mine{tenant_color_, color};
    boot_->Allgather(&mine, sizeof(TC), colors.data());
    std::vector<int> members;
    for (int i = 0; i < boot_size_; ++i)
        if (colors[i].tenant == tenant_color_ && colors[i].color == color && color >= 0)
            members.push_back(i);
    if (color < 0) members.clear();

    groups_.push_back(std::make_unique<ProcessGroup>(next_group_uid_++,
                                                     members.empty() ? std::vector<int>{boot_rank_} : members,
                                                     boot_rank_));
    ProcessGroup* g = groups_.back().get();
    // Collective over the WORLD (the unique-id exchange inside runs on the
    // bootstrap): every rank must call, members then init their comms.
    if (device_mode_) device_->EnsureGroupComms(g);
    return g;
}

void Context::FreeGroup(ProcessGroup* g) {
    // Groups are owned by the context and freed at Finalize; explicit free
    // just forgets device comms eagerly. (Persistent requests may outlive a
    // "freed" group handle in the reference too.)
    (void)g;
}

void* Context::Alloc(size_t size, size_t alignment) {
    if (alignment < 64) alignment = 64;
    void* p = nullptr;
    bool dev = device_mode_;
    if (dev) {
        p = device_->AllocDevice(size);
    } else {
        if (posix_memalign(&p, alignment, size) != 0) p = nullptr;
    }
    MLSL_CHECK(p != nullptr, "allocation failed");
    std::lock_guard<std::mutex> lk(alloc_mu_);
    allocs_[p] = AllocRec{size, dev};
    return p;
}

void Context::Free(void* ptr) {
    if (!ptr) return;
    bool dev = false;
    {
        std::lock_guard<std::mutex> lk(alloc_mu_);
        auto it = allocs_.find(ptr);
        MLSL_CHECK(it != allocs_.end(), "Free of unknown pointer");
        dev = it->second.device;
        allocs_.erase(it);
    }
    if (dev) device_->FreeDevice(ptr);
    else std::free(ptr);
}

bool Context::CheckBuffer(const void* ptr, size_t bytes) const {
    std::lock_guard<std::mutex> lk(alloc_mu_);
    for (const auto& kv : allocs_) {
        const char* base = static_cast<const char*>(kv.first);
        const char* p = static_cast<const char*>(ptr);
        if (p >= base && p + bytes <= base + kv.second.bytes) return true;
    }
    return false;
}

}  // namespace mlsl
