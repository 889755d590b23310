// C API for the standalone CDNA4 kernels (device-pointer in/out, used by
// the Python ops layer and GPU numerics tests). Synchronous variants run on
// the null stream and synchronize; the engine uses the stream variants
// internally.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../comm/context.hpp"
#include "../comm/device_comm.hpp"
#include "../comm/quant.hpp"
#include "../core/types.hpp"
#include "../hip/kernels.hpp"
#include "../include/mlsl/c_api.h"

using namespace mlsl;

extern "C" void mlsl_set_last_error_impl(const char* msg);

static void SyncNullStream() {
    if (hipStreamSynchronize(nullptr) != hipSuccess)
        throw Error("hipStreamSynchronize failed");
}

extern "C" {

#define OPS_TRY try {
#define OPS_CATCH                                                              \
    return MLSL_SUCCESS;                                                       \
    } catch (const std::exception& e) {                                        \
        mlsl_set_last_error_impl(e.what());                                    \
        return MLSL_FAILURE;                                                   \
    }

int mlsl_hip_device_count(int* out) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *out = n;
    return MLSL_SUCCESS;
}

int mlsl_set_compute_stream(void* stream) {
    OPS_TRY
    mlsl::DeviceRuntime* rt = mlsl::Context::Get().Device();
    if (rt) rt->SetComputeStream(stream);
    OPS_CATCH
}

int mlsl_hip_synchronize(void) {
    OPS_TRY if (hipDeviceSynchronize() != hipSuccess)
        throw Error("hipDeviceSynchronize failed");
    OPS_CATCH
}

int mlsl_hip_reduce(void* dst, const void* src, size_t count, int dt, int op) {
    OPS_TRY LaunchReduce(dst, src, count, static_cast<DataType>(dt),
                         static_cast<ReduceOp>(op), nullptr);
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_reduce_nt(void* dst, const void* src, size_t count) {
    OPS_TRY LaunchReduceNT(dst, src, count, nullptr);
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_reduce_nt2(void* dst, const void* src, size_t count) {
    OPS_TRY LaunchReduceNT2(dst, src, count, nullptr);
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_copy(void* dst, const void* src, size_t bytes) {
    OPS_TRY LaunchCopy(dst, src, bytes, nullptr);
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_copy_variant(void* dst, const void* src, size_t bytes, int nt) {
    OPS_TRY LaunchCopyVariant(dst, src, bytes, nt != 0, nullptr);
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_quantize(const void* in, void* err, void* wire, size_t count,
                      size_t block, int dt, int use_err) {
    OPS_TRY LaunchQuantize(in, err, wire, count, block, static_cast<DataType>(dt),
                           use_err != 0, nullptr);
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_dequantize(const void* wire, void* out, size_t count, size_t block, int dt) {
    OPS_TRY LaunchDequantize(wire, out, count, block, static_cast<DataType>(dt), nullptr);
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_quantize_f32_nt(const void* in, void* err, void* wire, size_t count,
                             size_t block) {
    OPS_TRY LaunchQuantizeF32NT(in, err, wire, count, block, nullptr);
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_dequantize_nt(const void* wire, void* out, size_t count, size_t block, int dt) {
    OPS_TRY LaunchDequantizeNT(wire, out, count, block, static_cast<DataType>(dt), nullptr);
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_quant_accum(void* acc, const void* wire, size_t count, size_t block) {
    OPS_TRY LaunchQuantAccum(acc, wire, count, block, nullptr);
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_quant_sum_dequant(const void* a_wire, const void* b_wire, void* out,
                               size_t count, size_t block, int dt) {
    OPS_TRY LaunchQuantSumDequant(a_wire, b_wire, out, count, block,
                                  static_cast<DataType>(dt), nullptr);
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_quant_sum_dequant_nt(const void* a_wire, const void* b_wire, void* out,
                                  size_t count, size_t block, int dt) {
    OPS_TRY LaunchQuantSumDequantNT(a_wire, b_wire, out, count, block,
                                    static_cast<DataType>(dt), nullptr);
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_quant_sum_dequant_n(const void* const* wires, int nwires, void* out,
                                 size_t count, size_t block, int dt) {
    OPS_TRY LaunchQuantSumDequantN(wires, nwires, out, count, block,
                                   static_cast<DataType>(dt), nullptr);
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_quant_sum_requant_n(const void* const* wires, int nwires, void* dst_wire,
                                 size_t nunits, size_t block) {
    OPS_TRY LaunchQuantSumRequantN(wires, nwires, dst_wire, nunits, block, nullptr);
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_dequantize_segments(const void* wire, size_t nseg, void* out, size_t count,
                                 size_t block, int dt, int accumulate) {
    OPS_TRY LaunchDequantizeSegments(wire, nseg, out, count, block,
                                     static_cast<DataType>(dt), accumulate != 0, nullptr);
    SyncNullStream();
    OPS_CATCH
}

}  // extern "C"

namespace {

// Prefix offsets of `counts`, every count checked; the total in *count.
std::vector<uint64_t> SegOffsets(const size_t* counts, size_t nseg, size_t* count,
                                 const char* where) {
    if (nseg == 0 || counts == nullptr)
        throw Error(std::string(where) + " takes at least one segment");
    std::vector<uint64_t> offs(nseg + 1, 0);
    for (size_t j = 0; j < nseg; ++j) {
        if (counts[j] == 0)
            throw Error(std::string(where) + ": segment " + std::to_string(j) + " is empty");
        offs[j + 1] = offs[j] + counts[j];
    }
    *count = offs[nseg];
    return offs;
}

// Both segment tables in one device allocation, for one synchronous op.
struct DevSegTables {
    void* mem = nullptr;
    const uint64_t* offs = nullptr;
    void** ptrs = nullptr;
    DevSegTables(const std::vector<uint64_t>& h_offs, const void* const* h_ptrs) {
        const size_t nseg = h_offs.size() - 1;
        const size_t ob = h_offs.size() * sizeof(uint64_t), pb = nseg * sizeof(void*);
        if (hipMalloc(&mem, ob + pb) != hipSuccess) throw Error("hipMalloc of segment tables");
        if (hipMemcpy(mem, h_offs.data(), ob, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(static_cast<uint8_t*>(mem) + ob, h_ptrs, pb, hipMemcpyHostToDevice) !=
                hipSuccess) {
            (void)hipFree(mem);
            throw Error("hipMemcpy of segment tables");
        }
        offs = static_cast<const uint64_t*>(mem);
        ptrs = reinterpret_cast<void**>(static_cast<uint8_t*>(mem) + ob);
    }
    ~DevSegTables() { (void)hipFree(mem); }
    DevSegTables(const DevSegTables&) = delete;
    DevSegTables& operator=(const DevSegTables&) = delete;
};

}  // namespace

extern "C" {

// The list-of-tensors codec: `ptrs` and `counts` are HOST arrays of nseg
// entries (device pointers in the hip variants, which upload both tables).
int mlsl_hip_quantize_gather(const void* const* ptrs, const size_t* counts, size_t nseg,
                             void* err, void* wire, size_t block, int dt, int use_err) {
    OPS_TRY CheckQuantBlock(block, "mlsl_hip_quantize_gather");
    size_t count = 0;
    const std::vector<uint64_t> offs = SegOffsets(counts, nseg, &count, "quantize-gather");
    DevSegTables tab(offs, ptrs);
    LaunchQuantizeGather(tab.ptrs, tab.offs, nseg, err, wire, count, block,
                         static_cast<DataType>(dt), use_err != 0, nullptr);
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_dequantize_scatter(const void* wire, void* const* ptrs, const size_t* counts,
                                size_t nseg, size_t block, int dt, float post_scale,
                                int round_first) {
    OPS_TRY CheckQuantBlock(block, "mlsl_hip_dequantize_scatter");
    size_t count = 0;
    const std::vector<uint64_t> offs = SegOffsets(counts, nseg, &count, "dequantize-scatter");
    DevSegTables tab(offs, ptrs);
    LaunchDequantizeScatter(wire, tab.ptrs, tab.offs, nseg, count, block,
                            static_cast<DataType>(dt), post_scale, round_first != 0, nullptr);
    SyncNullStream();
    OPS_CATCH
}

// The same two kernels over tables that already are in device memory (nseg + 1
// prefix offsets, nseg pointers), as a request keeps them: no upload here.
int mlsl_hip_quantize_gather_tables(const void* const* dev_ptrs, const uint64_t* dev_offs,
                                    size_t nseg, void* err, void* wire, size_t count,
                                    size_t block, int dt, int use_err) {
    OPS_TRY LaunchQuantizeGather(dev_ptrs, dev_offs, nseg, err, wire, count, block,
                                 static_cast<DataType>(dt), use_err != 0, nullptr);
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_dequantize_scatter_tables(const void* wire, void* const* dev_ptrs,
                                       const uint64_t* dev_offs, size_t nseg, size_t count,
                                       size_t block, int dt, float post_scale,
                                       int round_first) {
    OPS_TRY LaunchDequantizeScatter(wire, dev_ptrs, dev_offs, nseg, count, block,
                                    static_cast<DataType>(dt), post_scale, round_first != 0, nullptr);
    SyncNullStream();
    OPS_CATCH
}

// quantize-gather of the list padded with zeros to nshards * shard elements,
// shard by shard: wire j at wire + j * wire_stride, the residual flat.
int mlsl_hip_quantize_gather_shards(const void* const* ptrs, const size_t* counts, size_t nseg,
                                    void* err, void* wire, size_t nshards, size_t shard,
                                    size_t wire_stride, size_t block, int dt, int use_err) {
    OPS_TRY CheckQuantBlock(block, "mlsl_hip_quantize_gather_shards");
    size_t total = 0;
    const std::vector<uint64_t> offs =
        SegOffsets(counts, nseg, &total, "quantize-gather-shards");
    DevSegTables tab(offs, ptrs);
    LaunchQuantizeGatherShards(tab.ptrs, tab.offs, nseg, err, wire, total, nshards, shard,
                               wire_stride, block, static_cast<DataType>(dt), use_err != 0,
                               nullptr);
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_quantize_gather_shards_tables(const void* const* dev_ptrs,
                                           const uint64_t* dev_offs, size_t nseg, void* err,
                                           void* wire, size_t total, size_t nshards,
                                           size_t shard, size_t wire_stride, size_t block,
                                           int dt, int use_err) {
    OPS_TRY LaunchQuantizeGatherShards(dev_ptrs, dev_offs, nseg, err, wire, total, nshards,
                                       shard, wire_stride, block, static_cast<DataType>(dt),
                                       use_err != 0, nullptr);
    SyncNullStream();
    OPS_CATCH
}

int mlsl_host_quantize_gather_shards(const void* const* ptrs, const size_t* counts,
                                     size_t nseg, void* err, void* wire, size_t nshards,
                                     size_t shard, size_t wire_stride, size_t block, int dt,
                                     int use_err) {
    OPS_TRY CheckQuantBlock(block, "mlsl_host_quantize_gather_shards");
    size_t total = 0;
    const std::vector<uint64_t> offs =
        SegOffsets(counts, nseg, &total, "quantize-gather-shards");
    HostQuantizeGatherShards(ptrs, offs.data(), nseg, err, wire, total, nshards, shard,
                             wire_stride, block, static_cast<DataType>(dt), use_err != 0);
    OPS_CATCH
}

int mlsl_host_quantize_gather(const void* const* ptrs, const size_t* counts, size_t nseg,
                              void* err, void* wire, size_t block, int dt, int use_err) {
    OPS_TRY CheckQuantBlock(block, "mlsl_host_quantize_gather");
    size_t count = 0;
    const std::vector<uint64_t> offs = SegOffsets(counts, nseg, &count, "quantize-gather");
    HostQuantizeGather(ptrs, offs.data(), nseg, err, wire, count, block,
                       static_cast<DataType>(dt), use_err != 0);
    OPS_CATCH
}

int mlsl_host_dequantize_scatter(const void* wire, void* const* ptrs, const size_t* counts,
                                 size_t nseg, size_t block, int dt, float post_scale,
                                 int round_first) {
    OPS_TRY CheckQuantBlock(block, "mlsl_host_dequantize_scatter");
    size_t count = 0;
    const std::vector<uint64_t> offs = SegOffsets(counts, nseg, &count, "dequantize-scatter");
    HostDequantizeScatter(wire, ptrs, offs.data(), nseg, count, block,
                          static_cast<DataType>(dt), post_scale, round_first != 0);
    OPS_CATCH
}

// Host codec (comm/quant.cpp) on host pointers: same wire format and the
// same argument order as the device ops above.
int mlsl_host_quantize(const void* in, void* err, void* wire, size_t count,
                       size_t block, int dt, int use_err) {
    OPS_TRY CheckQuantBlock(block, "mlsl_host_quantize");
    HostQuantize(in, err, wire, count, block, static_cast<DataType>(dt), use_err != 0);
    OPS_CATCH
}

int mlsl_host_dequantize(const void* wire, void* out, size_t count, size_t block, int dt) {
    OPS_TRY CheckQuantBlock(block, "mlsl_host_dequantize");
    HostDequantize(wire, out, count, block, static_cast<DataType>(dt));
    OPS_CATCH
}

int mlsl_host_quant_accum(void* acc, const void* wire, size_t count, size_t block) {
    OPS_TRY CheckQuantBlock(block, "mlsl_host_quant_accum");
    HostQuantAccum(acc, wire, count, block);
    OPS_CATCH
}

int mlsl_host_quant_sum_dequant(const void* a_wire, const void* b_wire, void* out,
                                size_t count, size_t block, int dt) {
    OPS_TRY HostQuantSumDequant(a_wire, b_wire, out, count, block,
                                static_cast<DataType>(dt));
    OPS_CATCH
}

int mlsl_host_quant_sum_dequant_n(const void* const* wires, int nwires, void* out,
                                  size_t count, size_t block, int dt) {
    OPS_TRY HostQuantSumDequantN(wires, nwires, out, count, block,
                                 static_cast<DataType>(dt));
    OPS_CATCH
}

int mlsl_host_quant_sum_requant_n(const void* const* wires, int nwires, void* dst_wire,
                                  size_t nunits, size_t block) {
    OPS_TRY HostQuantSumRequantN(wires, nwires, dst_wire, nunits, block);
    OPS_CATCH
}

int mlsl_host_dequantize_segments(const void* wire, size_t nseg, void* out, size_t count,
                                  size_t block, int dt, int accumulate) {
    OPS_TRY HostDequantizeSegments(wire, nseg, out, count, block,
                                   static_cast<DataType>(dt), accumulate != 0);
    OPS_CATCH
}

int mlsl_hip_pack(const void* src, void* dst, size_t mb_off, size_t mb_cnt,
                  size_t fm_off, size_t fm_cnt, size_t fm_size, size_t buf_off,
                  size_t local_fm, size_t local_mb, int dt) {
    OPS_TRY PackBlockDesc d{mb_off, mb_cnt, fm_off, fm_cnt, fm_size, buf_off,
                            local_fm, local_mb};
    LaunchPack(src, dst, d, static_cast<DataType>(dt), nullptr);
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_unpack(const void* src, void* dst, size_t mb_off, size_t mb_cnt,
                    size_t fm_off, size_t fm_cnt, size_t fm_size, size_t buf_off,
                    size_t local_fm, size_t local_mb, int dt) {
    OPS_TRY PackBlockDesc d{mb_off, mb_cnt, fm_off, fm_cnt, fm_size, buf_off,
                            local_fm, local_mb};
    LaunchUnpack(src, dst, d, static_cast<DataType>(dt), nullptr);
    SyncNullStream();
    OPS_CATCH
}

}  // extern "C"
