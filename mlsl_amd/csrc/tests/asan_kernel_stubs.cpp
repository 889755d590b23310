// Host-only kernel-launcher stubs for the sanitizer builds: the CPU/TCP
// matrix never launches device kernels, but device_comm.cpp references the
// symbols. With g_kernel_trace null (the default) any call is a hard error.
// With a sink set (p2p_issue_trace.cpp) every call appends one line instead:
// the launcher's name, then each argument in hex, in declaration order.
// An XferPoll prints as {mbox target abort_word status max_ticks} or `null`,
// a FanPeer array as one {slot flag flag_val wait_mbox wait_target ctr
// ctr_target} per peer. The bool launchers answer as the real ones do.
#include <cstdio>
#include <string>
#include <type_traits>

#include "../core/types.hpp"
#include "../hip/kernels.hpp"

namespace mlsl {

std::string* g_kernel_trace = nullptr;

namespace {
struct Fan {
    const FanPeer* p;
    int n;
};

template <class T>
void Arg(std::string& o, T v) {
    unsigned long long x;
    if constexpr (std::is_pointer_v<T>) x = reinterpret_cast<uintptr_t>(v);
    else x = static_cast<unsigned long long>(v);
    char b[24];
    std::snprintf(b, sizeof b, " %llx", x);
    o += b;
}
void Arg(std::string& o, const XferPoll* p) {
    if (!p) {
        o += " null";
        return;
    }
    o += " {";
    Arg(o, p->mbox), Arg(o, p->target), Arg(o, p->abort_word), Arg(o, p->status);
    Arg(o, p->max_ticks);
    o += " }";
}
void Arg(std::string& o, Fan f) {
    for (int i = 0; i < f.n; ++i) {
        const FanPeer& q = f.p[i];
        o += " {";
        Arg(o, q.slot), Arg(o, q.flag), Arg(o, q.flag_val), Arg(o, q.wait_mbox);
        Arg(o, q.wait_target), Arg(o, q.ctr), Arg(o, q.ctr_target);
        o += " }";
    }
}
void Arg(std::string& o, const PackBlockDesc& d) {
    Arg(o, d.mb_offset), Arg(o, d.mb_count), Arg(o, d.fm_offset), Arg(o, d.fm_count);
    Arg(o, d.fm_size), Arg(o, d.buf_offset), Arg(o, d.local_fm_count), Arg(o, d.local_mb_count);
}

template <class... A>
void Record(const char* name, const A&... a) {
    if (!g_kernel_trace) MLSL_THROW("kernel launcher called in host-only ASan build");
    std::string& o = *g_kernel_trace;
    o += name;
    (Arg(o, a), ...);
    o += '\n';
}
bool Covered(DataType dt) { return dt == DataType::F32 || dt == DataType::BF16; }
}  // namespace

#define STUB(name, ...) { Record(#name, __VA_ARGS__); }
#define STUB_BOOL(ret, name, ...) { Record(#name, __VA_ARGS__); return ret; }
void LaunchReduce(void* d, const void* s, size_t n, DataType dt, ReduceOp op, hipStream_t st) STUB(LaunchReduce, d, s, n, dt, op, st)
void LaunchReduceNT(void* d, const void* s, size_t n, hipStream_t st) STUB(LaunchReduceNT, d, s, n, st)
void LaunchReduceNT2(void* d, const void* s, size_t n, hipStream_t st) STUB(LaunchReduceNT2, d, s, n, st)
void LaunchReduceOut(void* d, const void* a, const void* b, size_t n, DataType dt, ReduceOp op, hipStream_t st) STUB(LaunchReduceOut, d, a, b, n, dt, op, st)
void LaunchCopy(void* d, const void* s, size_t n, hipStream_t st) STUB(LaunchCopy, d, s, n, st)
void LaunchCopyVariant(void* d, const void* s, size_t n, bool nt, hipStream_t st) STUB(LaunchCopyVariant, d, s, n, nt, st)
void LaunchQuantize(const void* in, void* err, void* w, size_t n, size_t blk, DataType dt, bool use_err, hipStream_t st) STUB(LaunchQuantize, in, err, w, n, blk, dt, use_err, st)
void LaunchQuantizeF32NT(const void* in, void* err, void* w, size_t n, size_t blk, hipStream_t st) STUB(LaunchQuantizeF32NT, in, err, w, n, blk, st)
void LaunchDequantize(const void* w, void* out, size_t n, size_t blk, DataType dt, hipStream_t st) STUB(LaunchDequantize, w, out, n, blk, dt, st)
void LaunchDequantizeNT(const void* w, void* out, size_t n, size_t blk, DataType dt, hipStream_t st) STUB(LaunchDequantizeNT, w, out, n, blk, dt, st)
void LaunchQuantAccum(void* acc, const void* w, size_t n, size_t blk, hipStream_t st) STUB(LaunchQuantAccum, acc, w, n, blk, st)
void LaunchQuantSumDequant(const void* a, const void* b, void* out, size_t n, size_t blk, DataType dt, hipStream_t st) STUB(LaunchQuantSumDequant, a, b, out, n, blk, dt, st)
void LaunchQuantSumDequantNT(const void* a, const void* b, void* out, size_t n, size_t blk, DataType dt, hipStream_t st) STUB(LaunchQuantSumDequantNT, a, b, out, n, blk, dt, st)
void LaunchQuantSumDequantN(const void* const* w, int nw, void* out, size_t n, size_t blk, DataType dt, hipStream_t st) {
    Record("LaunchQuantSumDequantN", nw, out, n, blk, dt, st);
    for (int k = 0; k < nw; ++k) Record(" wire", w[k]);
}
void LaunchQuantSumRequantN(const void* const* w, int nw, void* dst, size_t units, size_t blk, hipStream_t st) {
    Record("LaunchQuantSumRequantN", nw, dst, units, blk, st);
    for (int k = 0; k < nw; ++k) Record(" wire", w[k]);
}
void LaunchDequantizeSegments(const void* w, size_t nseg, void* out, size_t n, size_t blk, DataType dt, bool acc, hipStream_t st) STUB(LaunchDequantizeSegments, w, nseg, out, n, blk, dt, acc, st)
void LaunchQuantizeGather(const void* const* ptrs, const uint64_t* offs, size_t nseg, void* err, void* w, size_t n, size_t blk, DataType dt, bool use_err, hipStream_t st) STUB(LaunchQuantizeGather, ptrs, offs, nseg, err, w, n, blk, dt, use_err, st)
void LaunchQuantizeGatherShards(const void* const* ptrs, const uint64_t* offs, size_t nseg, void* err, void* w, size_t total, size_t nshards, size_t shard, size_t stride, size_t blk, DataType dt, bool use_err, hipStream_t st) STUB(LaunchQuantizeGatherShards, ptrs, offs, nseg, err, w, total, nshards, shard, stride, blk, dt, use_err, st)
void LaunchDequantizeScatter(const void* w, void* const* ptrs, const uint64_t* offs, size_t nseg, size_t n, size_t blk, DataType dt, float post, bool round_first, hipStream_t st) STUB(LaunchDequantizeScatter, w, ptrs, offs, nseg, n, blk, dt, post, round_first, st)
void LaunchPack(const void* s, void* d, const PackBlockDesc& pd, DataType dt, hipStream_t st) STUB(LaunchPack, s, d, pd, dt, st)
void LaunchUnpack(const void* s, void* d, const PackBlockDesc& pd, DataType dt, hipStream_t st) STUB(LaunchUnpack, s, d, pd, dt, st)
void LaunchWaitFlag(const void* mbox, uint64_t target, const void* abort_word, void* status, uint64_t max_ticks, hipStream_t st) STUB(LaunchWaitFlag, mbox, target, abort_word, status, max_ticks, st)
void LaunchSetFlag(void* mbox, uint64_t val, hipStream_t st) STUB(LaunchSetFlag, mbox, val, st)
void LaunchXferCopy(void* d, const void* s, size_t n, const XferPoll* poll, hipStream_t st) STUB(LaunchXferCopy, d, s, n, poll, st)
void LaunchXferSendFused(void* slot, const void* src, size_t n, const XferPoll* bp, void* ctr, uint64_t ctr_target, void* in_mbox, uint64_t seq, hipStream_t st) STUB(LaunchXferSendFused, slot, src, n, bp, ctr, ctr_target, in_mbox, seq, st)
bool LaunchXferRecvFused(void* d, const void* slot, const void* other, size_t n, DataType dt, ReduceOp op, FusedConsume mode, const XferPoll* wp, void* ctr, uint64_t ctr_target, void* ack_mbox, uint64_t seq, hipStream_t st) STUB_BOOL(mode == FusedConsume::COPY || Covered(dt), LaunchXferRecvFused, d, slot, other, n, dt, op, mode, wp, ctr, ctr_target, ack_mbox, seq, st)
int FanOutWgsPerPeer(int npeers) { return npeers <= 1 ? 32 : npeers <= 4 ? 8 : 4; }
void LaunchXferRecvQuantAccum(void* acc, const void* slot, size_t n, size_t blk, const XferPoll* wp, void* ctr, uint64_t ctr_target, void* ack_mbox, uint64_t seq, hipStream_t st) STUB(LaunchXferRecvQuantAccum, acc, slot, n, blk, wp, ctr, ctr_target, ack_mbox, seq, st)
void LaunchFanOutSend(const void* src, size_t n, const FanPeer* peers, int np, const XferPoll* ab, hipStream_t st) STUB(LaunchFanOutSend, src, n, Fan{peers, np}, np, ab, st)
bool LaunchFanInReduce(void* d, size_t n, DataType dt, ReduceOp op, const FanPeer* peers, int np, void* ctr, uint64_t ctr_target, const XferPoll* ab, hipStream_t st) STUB_BOOL(Covered(dt), LaunchFanInReduce, d, n, dt, op, Fan{peers, np}, np, ctr, ctr_target, ab, st)
bool LaunchXferReduce(void* d, const void* slot, const void* other, size_t n, DataType dt, ReduceOp op, const XferPoll* poll, hipStream_t st) STUB_BOOL(Covered(dt), LaunchXferReduce, d, slot, other, n, dt, op, poll, st)
}  // namespace mlsl
