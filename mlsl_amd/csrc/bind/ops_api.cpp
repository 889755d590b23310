// C API for the standalone CDNA4 kernels (device-pointer in/out, used by
// the Python ops layer and GPU numerics tests). Synchronous variants run on
// the null stream and synchronize; the engine uses the stream variants
// internally.
#include <hip/hip_runtime.h>

#include <cstring>
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

// The int4 codec. path: 0 lets the launcher choose, 1 names the generic
// kernel, 2 the fast one (an error where it does not apply).
int mlsl_hip_quantize4(const void* in, void* err, void* wire, size_t count, size_t block,
                       int dt, int use_err, int path) {
    OPS_TRY LaunchQuantize4(in, err, wire, count, block, static_cast<DataType>(dt),
                            use_err != 0, nullptr, static_cast<Quant4Path>(path));
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_dequantize4(const void* wire, void* out, size_t count, size_t block, int dt,
                         int path) {
    OPS_TRY LaunchDequantize4(wire, out, count, block, static_cast<DataType>(dt), nullptr,
                              static_cast<Quant4Path>(path));
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_quant_sum_dequant_n4(const void* const* wires, int nwires, void* out,
                                  size_t count, size_t block, int dt, int path) {
    OPS_TRY LaunchQuantSumDequantN4(wires, nwires, out, count, block,
                                    static_cast<DataType>(dt), nullptr,
                                    static_cast<Quant4Path>(path));
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_quant_sum_requant_n4(const void* const* wires, int nwires, void* dst_wire,
                                  size_t nunits, size_t block, int path) {
    OPS_TRY LaunchQuantSumRequantN4(wires, nwires, dst_wire, nunits, block, nullptr,
                                    static_cast<Quant4Path>(path));
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_quant4_blocks_per_trip(int fast, size_t* out) {
    OPS_TRY* out = Quant4BlocksPerTrip(fast != 0);
    OPS_CATCH
}

int mlsl_host_quantize4(const void* in, void* err, void* wire, size_t count, size_t block,
                        int dt, int use_err) {
    OPS_TRY HostQuantize(in, err, wire, count, block, static_cast<DataType>(dt), use_err != 0,
                         4);
    OPS_CATCH
}

int mlsl_host_dequantize4(const void* wire, void* out, size_t count, size_t block, int dt) {
    OPS_TRY HostDequantize(wire, out, count, block, static_cast<DataType>(dt), 4);
    OPS_CATCH
}

int mlsl_host_quant_sum_dequant_n4(const void* const* wires, int nwires, void* out,
                                   size_t count, size_t block, int dt) {
    OPS_TRY HostQuantSumDequantN(wires, nwires, out, count, block, static_cast<DataType>(dt),
                                 4);
    OPS_CATCH
}

int mlsl_host_quant_sum_requant_n4(const void* const* wires, int nwires, void* dst_wire,
                                   size_t nunits, size_t block) {
    OPS_TRY HostQuantSumRequantN(wires, nwires, dst_wire, nunits, block, 4);
    OPS_CATCH
}

int mlsl_hip_dequantize_segments(const void* wire, size_t nseg, void* out, size_t count,
                                 size_t block, int dt, int accumulate) {
    OPS_TRY LaunchDequantizeSegments(wire, nseg, out, count, block,
                                     static_cast<DataType>(dt), accumulate != 0, nullptr);
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_dequantize_segments4(const void* wire, size_t nseg, void* out, size_t count,
                                  size_t block, int dt, int accumulate, int path) {
    OPS_TRY LaunchDequantizeSegments4(wire, nseg, out, count, block,
                                      static_cast<DataType>(dt), accumulate != 0, nullptr,
                                      static_cast<Quant4Path>(path));
    SyncNullStream();
    OPS_CATCH
}

int mlsl_host_dequantize_segments4(const void* wire, size_t nseg, void* out, size_t count,
                                   size_t block, int dt, int accumulate) {
    OPS_TRY HostDequantizeSegments(wire, nseg, out, count, block,
                                   static_cast<DataType>(dt), accumulate != 0, 4);
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

// The list codec on the int4 wire; path as in mlsl_hip_quantize4.
int mlsl_hip_quantize_gather4(const void* const* ptrs, const size_t* counts, size_t nseg,
                              void* err, void* wire, size_t block, int dt, int use_err,
                              int path) {
    OPS_TRY CheckQuantBlock(block, "mlsl_hip_quantize_gather4", 4);
    size_t count = 0;
    const std::vector<uint64_t> offs = SegOffsets(counts, nseg, &count, "quantize-gather");
    DevSegTables tab(offs, ptrs);
    LaunchQuantizeGather4(tab.ptrs, tab.offs, nseg, err, wire, count, block,
                          static_cast<DataType>(dt), use_err != 0, nullptr,
                          static_cast<Quant4Path>(path));
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_dequantize_scatter4(const void* wire, void* const* ptrs, const size_t* counts,
                                 size_t nseg, size_t block, int dt, float post_scale,
                                 int round_first, int path) {
    OPS_TRY CheckQuantBlock(block, "mlsl_hip_dequantize_scatter4", 4);
    size_t count = 0;
    const std::vector<uint64_t> offs = SegOffsets(counts, nseg, &count, "dequantize-scatter");
    DevSegTables tab(offs, ptrs);
    LaunchDequantizeScatter4(wire, tab.ptrs, tab.offs, nseg, count, block,
                             static_cast<DataType>(dt), post_scale, round_first != 0, nullptr,
                             static_cast<Quant4Path>(path));
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_quantize_gather4_tables(const void* const* dev_ptrs, const uint64_t* dev_offs,
                                     size_t nseg, void* err, void* wire, size_t count,
                                     size_t block, int dt, int use_err, int path) {
    OPS_TRY LaunchQuantizeGather4(dev_ptrs, dev_offs, nseg, err, wire, count, block,
                                  static_cast<DataType>(dt), use_err != 0, nullptr,
                                  static_cast<Quant4Path>(path));
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_dequantize_scatter4_tables(const void* wire, void* const* dev_ptrs,
                                        const uint64_t* dev_offs, size_t nseg, size_t count,
                                        size_t block, int dt, float post_scale,
                                        int round_first, int path) {
    OPS_TRY LaunchDequantizeScatter4(wire, dev_ptrs, dev_offs, nseg, count, block,
                                     static_cast<DataType>(dt), post_scale, round_first != 0,
                                     nullptr, static_cast<Quant4Path>(path));
    SyncNullStream();
    OPS_CATCH
}

int mlsl_host_quantize_gather4(const void* const* ptrs, const size_t* counts, size_t nseg,
                               void* err, void* wire, size_t block, int dt, int use_err) {
    OPS_TRY CheckQuantBlock(block, "mlsl_host_quantize_gather4", 4);
    size_t count = 0;
    const std::vector<uint64_t> offs = SegOffsets(counts, nseg, &count, "quantize-gather");
    HostQuantizeGather(ptrs, offs.data(), nseg, err, wire, count, block,
                       static_cast<DataType>(dt), use_err != 0, 4);
    OPS_CATCH
}

int mlsl_host_dequantize_scatter4(const void* wire, void* const* ptrs, const size_t* counts,
                                  size_t nseg, size_t block, int dt, float post_scale,
                                  int round_first) {
    OPS_TRY CheckQuantBlock(block, "mlsl_host_dequantize_scatter4", 4);
    size_t count = 0;
    const std::vector<uint64_t> offs = SegOffsets(counts, nseg, &count, "dequantize-scatter");
    HostDequantizeScatter(wire, ptrs, offs.data(), nseg, count, block,
                          static_cast<DataType>(dt), post_scale, round_first != 0, 4);
    OPS_CATCH
}

// The exact pair: the list copied into `flat`, and `flat` scaled back into it.
int mlsl_hip_gather_list(const void* const* ptrs, const size_t* counts, size_t nseg,
                         void* flat, int dt) {
    OPS_TRY size_t count = 0;
    const std::vector<uint64_t> offs = SegOffsets(counts, nseg, &count, "gather-list");
    DevSegTables tab(offs, ptrs);
    LaunchGatherList(tab.ptrs, tab.offs, nseg, flat, count, static_cast<DataType>(dt), nullptr);
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_scatter_scale_list(const void* flat, void* const* ptrs, const size_t* counts,
                                size_t nseg, int dt, float post_scale) {
    OPS_TRY size_t count = 0;
    const std::vector<uint64_t> offs = SegOffsets(counts, nseg, &count, "scatter-scale-list");
    DevSegTables tab(offs, ptrs);
    LaunchScatterScaleList(flat, tab.ptrs, tab.offs, nseg, count, static_cast<DataType>(dt),
                           post_scale, nullptr);
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_gather_list_tables(const void* const* dev_ptrs, const uint64_t* dev_offs,
                                size_t nseg, void* flat, size_t count, int dt) {
    OPS_TRY LaunchGatherList(dev_ptrs, dev_offs, nseg, flat, count, static_cast<DataType>(dt),
                             nullptr);
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_scatter_scale_list_tables(const void* flat, void* const* dev_ptrs,
                                       const uint64_t* dev_offs, size_t nseg, size_t count,
                                       int dt, float post_scale) {
    OPS_TRY LaunchScatterScaleList(flat, dev_ptrs, dev_offs, nseg, count,
                                   static_cast<DataType>(dt), post_scale, nullptr);
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_list_elems_per_trip(int dt, size_t* out) {
    OPS_TRY* out = ListElemsPerTrip(static_cast<DataType>(dt));
    OPS_CATCH
}

// Clipping by the global norm: `out` and `total` are one double in DEVICE
// memory; the sum of squares goes there and the scale reads it from there.
int mlsl_hip_sumsq(const void* in, size_t count, int dt, double* out, int accumulate) {
    OPS_TRY LaunchSumSq(in, count, static_cast<DataType>(dt), out, accumulate != 0, nullptr);
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_sumsq_list(const void* const* ptrs, const size_t* counts, size_t nseg, int dt,
                        double* out, int accumulate) {
    OPS_TRY size_t count = 0;
    const std::vector<uint64_t> offs = SegOffsets(counts, nseg, &count, "sumsq-list");
    DevSegTables tab(offs, ptrs);
    LaunchSumSqList(tab.ptrs, tab.offs, nseg, count, static_cast<DataType>(dt), out,
                    accumulate != 0, nullptr);
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_sumsq_list_tables(const void* const* dev_ptrs, const uint64_t* dev_offs,
                               size_t nseg, size_t count, int dt, double* out,
                               int accumulate) {
    OPS_TRY LaunchSumSqList(dev_ptrs, dev_offs, nseg, count, static_cast<DataType>(dt), out,
                            accumulate != 0, nullptr);
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_clip_scale(void* data, size_t count, int dt, const double* total,
                        float max_norm) {
    OPS_TRY LaunchClipScale(data, count, static_cast<DataType>(dt), total, max_norm, nullptr);
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_clip_scale_list(void* const* ptrs, const size_t* counts, size_t nseg, int dt,
                             const double* total, float max_norm) {
    OPS_TRY size_t count = 0;
    const std::vector<uint64_t> offs = SegOffsets(counts, nseg, &count, "clip-scale-list");
    DevSegTables tab(offs, ptrs);
    LaunchClipScaleList(tab.ptrs, tab.offs, nseg, count, static_cast<DataType>(dt), total,
                        max_norm, nullptr);
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_clip_scale_list_tables(void* const* dev_ptrs, const uint64_t* dev_offs,
                                    size_t nseg, size_t count, int dt, const double* total,
                                    float max_norm) {
    OPS_TRY LaunchClipScaleList(dev_ptrs, dev_offs, nseg, count, static_cast<DataType>(dt),
                                total, max_norm, nullptr);
    SyncNullStream();
    OPS_CATCH
}

// The fused AdamW step. `scalars` is the ten floats of AdamWScalars in its
// order; `total` (may be null) is one double, in DEVICE memory for the device
// form and in host memory for the host twin.
int mlsl_hip_adamw_step(const void* g, void* p, void* m, void* v, void* out,
                        const void* replica, size_t count, int dt, const double* total,
                        const float* scalars, int path) {
    OPS_TRY AdamWScalars s;
    std::memcpy(&s, scalars, sizeof s);
    LaunchAdamWStep(g, static_cast<float*>(p), static_cast<float*>(m), static_cast<float*>(v),
                    out, replica, count, static_cast<DataType>(dt), total, s, nullptr,
                    static_cast<Quant4Path>(path));
    SyncNullStream();
    OPS_CATCH
}

int mlsl_host_adamw_step(const void* g, void* p, void* m, void* v, void* out,
                         const void* replica, size_t count, int dt, const double* total,
                         const float* scalars) {
    OPS_TRY AdamWScalars s;
    std::memcpy(&s, scalars, sizeof s);
    HostAdamWStep(g, static_cast<float*>(p), static_cast<float*>(m), static_cast<float*>(v), out,
                  replica, count, static_cast<DataType>(dt), total, s);
    OPS_CATCH
}

int mlsl_hip_adamw_elems_per_trip(size_t* out) {
    OPS_TRY* out = AdamWElemsPerTrip();
    OPS_CATCH
}

int mlsl_host_gather_list(const void* const* ptrs, const size_t* counts, size_t nseg,
                          void* flat, int dt) {
    OPS_TRY size_t count = 0;
    const std::vector<uint64_t> offs = SegOffsets(counts, nseg, &count, "gather-list");
    HostGatherList(ptrs, offs.data(), nseg, flat, count, static_cast<DataType>(dt));
    OPS_CATCH
}

int mlsl_host_scatter_scale_list(const void* flat, void* const* ptrs, const size_t* counts,
                                 size_t nseg, int dt, float post_scale) {
    OPS_TRY size_t count = 0;
    const std::vector<uint64_t> offs = SegOffsets(counts, nseg, &count, "scatter-scale-list");
    HostScatterScaleList(flat, ptrs, offs.data(), nseg, count, static_cast<DataType>(dt),
                         post_scale);
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

// The same three on the int4 wire; path as in mlsl_hip_quantize4.
int mlsl_hip_quantize_gather_shards4(const void* const* ptrs, const size_t* counts,
                                     size_t nseg, void* err, void* wire, size_t nshards,
                                     size_t shard, size_t wire_stride, size_t block, int dt,
                                     int use_err, int path) {
    OPS_TRY CheckQuantBlock(block, "mlsl_hip_quantize_gather_shards4", 4);
    size_t total = 0;
    const std::vector<uint64_t> offs =
        SegOffsets(counts, nseg, &total, "quantize-gather-shards");
    DevSegTables tab(offs, ptrs);
    LaunchQuantizeGatherShards4(tab.ptrs, tab.offs, nseg, err, wire, total, nshards, shard,
                                wire_stride, block, static_cast<DataType>(dt), use_err != 0,
                                nullptr, static_cast<Quant4Path>(path));
    SyncNullStream();
    OPS_CATCH
}

int mlsl_hip_quantize_gather_shards4_tables(const void* const* dev_ptrs,
                                            const uint64_t* dev_offs, size_t nseg, void* err,
                                            void* wire, size_t total, size_t nshards,
                                            size_t shard, size_t wire_stride, size_t block,
                                            int dt, int use_err, int path) {
    OPS_TRY LaunchQuantizeGatherShards4(dev_ptrs, dev_offs, nseg, err, wire, total, nshards,
                                        shard, wire_stride, block, static_cast<DataType>(dt),
                                        use_err != 0, nullptr, static_cast<Quant4Path>(path));
    SyncNullStream();
    OPS_CATCH
}

int mlsl_host_quantize_gather_shards4(const void* const* ptrs, const size_t* counts,
                                      size_t nseg, void* err, void* wire, size_t nshards,
                                      size_t shard, size_t wire_stride, size_t block, int dt,
                                      int use_err) {
    OPS_TRY CheckQuantBlock(block, "mlsl_host_quantize_gather_shards4", 4);
    size_t total = 0;
    const std::vector<uint64_t> offs =
        SegOffsets(counts, nseg, &total, "quantize-gather-shards");
    HostQuantizeGatherShards(ptrs, offs.data(), nseg, err, wire, total, nshards, shard,
                             wire_stride, block, static_cast<DataType>(dt), use_err != 0, 4);
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
