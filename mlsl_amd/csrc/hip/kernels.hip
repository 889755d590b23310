// CDNA4 (gfx950) kernels for the communication hot path: local reductions
// for the schedule-driven collectives, int8 block quantization with error
// feedback, and pack/unpack between layer layouts and comm buffers.
//
// Design per the MI355X rules: 64-wide wavefronts, 256-thread blocks,
// 16-byte vectorized accesses where alignment permits, grid capped at
// ~8 blocks/CU with grid-stride loops (memory-bound ops: HBM3E is the
// roofline, not VALU).
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "../core/log.hpp"
#include "kernels.hpp"

namespace mlsl {

#define HIP_CHECK(cmd)                                                        \
    do {                                                                      \
        hipError_t e_ = (cmd);                                                \
        if (e_ != hipSuccess)                                                 \
            MLSL_THROW(std::string("HIP error: ") + hipGetErrorString(e_));   \
    } while (0)

namespace {

constexpr int kBlock = 256;
// 256 CUs × 8 blocks/CU: enough residency to cover HBM latency without
// oversubscribing the launch path.
constexpr int kMaxGrid = 2048;

inline int GridFor(size_t work_items) {
    size_t g = (work_items + kBlock - 1) / kBlock;
    if (g > kMaxGrid) g = kMaxGrid;
    if (g == 0) g = 1;
    return static_cast<int>(g);
}

// Runtime value -> compile-time instantiation: f receives the value as a
// std::integral_constant and reads it back with decltype(x)::value.
template <typename F>
void DispatchOp(ReduceOp op, F&& f) {
    switch (op) {
        case ReduceOp::SUM: f(std::integral_constant<ReduceOp, ReduceOp::SUM>{}); break;
        case ReduceOp::MIN: f(std::integral_constant<ReduceOp, ReduceOp::MIN>{}); break;
        case ReduceOp::MAX: f(std::integral_constant<ReduceOp, ReduceOp::MAX>{}); break;
    }
}

template <typename F>
void DispatchBool(bool b, F&& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

using float4_ev = __attribute__((ext_vector_type(4))) float;
using uint2_ev = __attribute__((ext_vector_type(2))) unsigned int;
using uint4_ev = __attribute__((ext_vector_type(4))) unsigned int;
using ushort4_t = __attribute__((ext_vector_type(4))) unsigned short;
using ushort8_t = __attribute__((ext_vector_type(8))) unsigned short;

// ---- element codec ----
// `unsigned short` is the bf16 container everywhere in this file. bf16 and
// f16 do their arithmetic in float; every other type is its own arithmetic
// type.
template <typename T> struct Arith { using type = T; };
template <> struct Arith<unsigned short> { using type = float; };
template <> struct Arith<__half> { using type = float; };
template <typename T> using ArithT = typename Arith<T>::type;

template <typename T>
__device__ __forceinline__ ArithT<T> Decode(T v) {
    if constexpr (std::is_same_v<T, unsigned short>)
        return __bfloat162float(__hip_bfloat16_raw{v});
    else if constexpr (std::is_same_v<T, __half>)
        return __half2float(v);
    else
        return v;
}

template <typename T>
__device__ __forceinline__ T Encode(ArithT<T> v) {
    if constexpr (std::is_same_v<T, unsigned short>) {
        __hip_bfloat16 h = __float2bfloat16(v);
        return reinterpret_cast<unsigned short&>(h);
    } else if constexpr (std::is_same_v<T, __half>) {
        return __float2half(v);
    } else {
        return v;
    }
}

template <typename T, ReduceOp OP>
__device__ __forceinline__ T Apply(T a, T b) {
    if constexpr (OP == ReduceOp::SUM) return a + b;
    if constexpr (OP == ReduceOp::MIN) return a < b ? a : b;
    return a > b ? a : b;
}

template <typename T, ReduceOp OP>
__device__ __forceinline__ T Combine(T a, T b) {
    return Encode<T>(Apply<ArithT<T>, OP>(Decode(a), Decode(b)));
}

// Lane-wise Combine over an ext-vector of N elements.
template <typename T, ReduceOp OP, int N, typename V>
__device__ __forceinline__ V CombineVec(V a, V b) {
#pragma unroll
    for (int j = 0; j < N; ++j) a[j] = Combine<T, OP>(a[j], b[j]);
    return a;
}

// ---- f32 in-place reduce; the loop shape is a template argument so the
// A/B variants share prologue and tail ----
//   UNROLL2: float4, 2-deep strided unroll for MLP (default policy)
//   NT:      one float4 per iteration, nontemporal (bypass L2 retention)
//   NT2:     two consecutive float4 (32 B/lane) per iteration, nontemporal
enum class F32Loop { UNROLL2, NT, NT2 };

template <ReduceOp OP, F32Loop LOOP>
__global__ void ReduceF32Kernel(float* __restrict__ dst,
                                const float* __restrict__ src, size_t n) {
    const size_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = gridDim.x * blockDim.x;
    const float4_ev* s4 = reinterpret_cast<const float4_ev*>(src);
    float4_ev* d4 = reinterpret_cast<float4_ev*>(dst);
    size_t done;  // elements covered by the vector loop
    if constexpr (LOOP == F32Loop::UNROLL2) {
        const size_t n4 = n / 4;
        size_t i = tid;
        for (; i + stride < n4; i += 2 * stride) {
            float4_ev a0 = d4[i], b0 = s4[i];
            float4_ev a1 = d4[i + stride], b1 = s4[i + stride];
            d4[i] = CombineVec<float, OP, 4>(a0, b0);
            d4[i + stride] = CombineVec<float, OP, 4>(a1, b1);
        }
        for (; i < n4; i += stride)
            d4[i] = CombineVec<float, OP, 4>(d4[i], s4[i]);
        done = n4 * 4;
    } else if constexpr (LOOP == F32Loop::NT) {
        const size_t n4 = n / 4;
        for (size_t i = tid; i < n4; i += stride) {
            float4_ev a = __builtin_nontemporal_load(d4 + i);
            float4_ev b = __builtin_nontemporal_load(s4 + i);
            __builtin_nontemporal_store(CombineVec<float, OP, 4>(a, b), d4 + i);
        }
        done = n4 * 4;
    } else {
        const size_t n8 = n / 8;
        for (size_t i = tid; i < n8; i += stride) {
            float4_ev a0 = __builtin_nontemporal_load(d4 + 2 * i);
            float4_ev a1 = __builtin_nontemporal_load(d4 + 2 * i + 1);
            float4_ev b0 = __builtin_nontemporal_load(s4 + 2 * i);
            float4_ev b1 = __builtin_nontemporal_load(s4 + 2 * i + 1);
            __builtin_nontemporal_store(CombineVec<float, OP, 4>(a0, b0), d4 + 2 * i);
            __builtin_nontemporal_store(CombineVec<float, OP, 4>(a1, b1), d4 + 2 * i + 1);
        }
        done = n8 * 8;
    }
    for (size_t j = done + tid; j < n; j += stride)
        dst[j] = Apply<float, OP>(dst[j], src[j]);
}

// ---- generic scalar reduce (f16/f64/i32/i64/u8) ----
template <typename T, ReduceOp OP>
__global__ void ReduceScalarKernel(T* __restrict__ dst, const T* __restrict__ src,
                                   size_t n) {
    const size_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = gridDim.x * blockDim.x;
    for (size_t i = tid; i < n; i += stride)
        dst[i] = Combine<T, OP>(dst[i], src[i]);
}

// ---- bf16: 4-element (8 B) vectors + scalar tail ----
template <ReduceOp OP>
__global__ void ReduceBf16Kernel(unsigned short* __restrict__ dst,
                                 const unsigned short* __restrict__ src, size_t n) {
    const size_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = gridDim.x * blockDim.x;
    const size_t n4 = n / 4;
    const ushort4_t* s4 = reinterpret_cast<const ushort4_t*>(src);
    ushort4_t* d4 = reinterpret_cast<ushort4_t*>(dst);
    for (size_t i = tid; i < n4; i += stride)
        d4[i] = CombineVec<unsigned short, OP, 4>(d4[i], s4[i]);
    for (size_t i = n4 * 4 + tid; i < n; i += stride)
        dst[i] = Combine<unsigned short, OP>(dst[i], src[i]);
}

template <typename T, typename Kern>
void RunReduce(Kern kern, size_t work_items, void* dst, const void* src, size_t n,
               hipStream_t stream) {
    kern<<<dim3(GridFor(work_items)), dim3(kBlock), 0, stream>>>(
        static_cast<T*>(dst), static_cast<const T*>(src), n);
}

}  // namespace

void LaunchReduce(void* dst, const void* src, size_t count, DataType dt,
                  ReduceOp op, hipStream_t stream) {
    // Nontemporal path for f32 streams past L2 reach: measured 4.2 -> 5.3
    // TB/s on 256 MiB (docs/BENCHMARKS.md); bf16 measured slower with NT
    // (5.64 -> 5.01 TB/s) and keeps the default policy.
    const bool nt = count * DtypeSize(dt) >= (16u << 20);
    const size_t vec = count / 4 + 1;
    DispatchOp(op, [&](auto o) {
        constexpr ReduceOp OP = decltype(o)::value;
        switch (dt) {
            case DataType::F32:
                if (nt) RunReduce<float>(ReduceF32Kernel<OP, F32Loop::NT>, vec, dst, src, count, stream);
                else RunReduce<float>(ReduceF32Kernel<OP, F32Loop::UNROLL2>, vec, dst, src, count, stream);
                break;
            case DataType::BF16:
                RunReduce<unsigned short>(ReduceBf16Kernel<OP>, vec, dst, src, count, stream);
                break;
            case DataType::F16:
                RunReduce<__half>(ReduceScalarKernel<__half, OP>, vec, dst, src, count, stream);
                break;
            case DataType::F64:
                RunReduce<double>(ReduceScalarKernel<double, OP>, count, dst, src, count, stream);
                break;
            case DataType::U8:
                RunReduce<uint8_t>(ReduceScalarKernel<uint8_t, OP>, count, dst, src, count, stream);
                break;
            case DataType::I32:
                RunReduce<int32_t>(ReduceScalarKernel<int32_t, OP>, count, dst, src, count, stream);
                break;
            case DataType::I64:
                RunReduce<int64_t>(ReduceScalarKernel<int64_t, OP>, count, dst, src, count, stream);
                break;
        }
    });
    HIP_CHECK(hipGetLastError());
}

void LaunchReduceNT(void* dst, const void* src, size_t count, hipStream_t stream) {
    RunReduce<float>(ReduceF32Kernel<ReduceOp::SUM, F32Loop::NT>, count / 4 + 1, dst,
                     src, count, stream);
    HIP_CHECK(hipGetLastError());
}

void LaunchReduceNT2(void* dst, const void* src, size_t count, hipStream_t stream) {
    RunReduce<float>(ReduceF32Kernel<ReduceOp::SUM, F32Loop::NT2>, count / 4 + 1, dst,
                     src, count, stream);
    HIP_CHECK(hipGetLastError());
}

namespace {

// Streaming copy: 16-B lanes, 2-deep unroll. NT template arm bypasses L2
// retention (each XCD's L2 is private; retention buys nothing for a pure
// copy) — A/B-measured against plain accesses.
template <bool NT>
__global__ void CopyNTKernel(uint4_ev* __restrict__ dst,
                             const uint4_ev* __restrict__ src, size_t n16) {
    const size_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = gridDim.x * blockDim.x;
    size_t i = tid;
    for (; i + stride < n16; i += 2 * stride) {
        uint4_ev a, b;
        if constexpr (NT) {
            a = __builtin_nontemporal_load(src + i);
            b = __builtin_nontemporal_load(src + i + stride);
            __builtin_nontemporal_store(a, dst + i);
            __builtin_nontemporal_store(b, dst + i + stride);
        } else {
            a = src[i];
            b = src[i + stride];
            dst[i] = a;
            dst[i + stride] = b;
        }
    }
    for (; i < n16; i += stride) {
        if constexpr (NT)
            __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + i);
        else
            dst[i] = src[i];
    }
}

}  // namespace

void LaunchCopyVariant(void* dst, const void* src, size_t bytes, bool nt,
                       hipStream_t stream) {
    const uintptr_t d = reinterpret_cast<uintptr_t>(dst);
    const uintptr_t s = reinterpret_cast<uintptr_t>(src);
    // Kernel path: 16-B aligned and big enough that launch cost (~5 us)
    // amortizes against the bandwidth win over the blit path.
    if (((d | s | bytes) & 15) == 0 && bytes >= (1u << 20)) {
        const size_t n16 = bytes / 16;
        DispatchBool(nt, [&](auto v) {
            CopyNTKernel<decltype(v)::value><<<dim3(GridFor(n16)), dim3(kBlock), 0, stream>>>(
                static_cast<uint4_ev*>(dst), static_cast<const uint4_ev*>(src), n16);
        });
        HIP_CHECK(hipGetLastError());
        return;
    }
    HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream));
}

void LaunchCopy(void* dst, const void* src, size_t bytes, hipStream_t stream) {
    LaunchCopyVariant(dst, src, bytes, /*nt=*/true, stream);
}

void LaunchReduceOut(void* dst, const void* a, const void* b, size_t count,
                     DataType dt, ReduceOp op, hipStream_t stream) {
    // dst = a; dst += b  (two passes is fine: memory-bound and rarely used;
    // the in-place variant is the hot one).
    HIP_CHECK(hipMemcpyAsync(dst, a, count * DtypeSize(dt), hipMemcpyDeviceToDevice, stream));
    LaunchReduce(dst, b, count, dt, op, stream);
}

// ---------------------------------------------------------------------------
// int8 block quantization with error feedback.
// Wire block: [float scale][float reserved][int8 x block_elems], 8-byte header.

namespace {

constexpr size_t kWireHdr = 8;
// The two-blocks-per-wave and register-resident fast paths are built for
// this block size.
constexpr size_t kFastBlock = 256;

// ---- int8 block codec ----
__device__ __forceinline__ float QScale(float block_max) {
    return block_max > 0.f ? block_max / 127.f : 1.f;
}
__device__ __forceinline__ float QRound(float v, float inv_scale) {
    return fminf(127.f, fmaxf(-127.f, nearbyintf(v * inv_scale)));
}
// byte j of a packed word <-> one quantized value
__device__ __forceinline__ uint32_t QPack(float q, int j) {
    return (static_cast<uint32_t>(static_cast<int32_t>(q)) & 0xffu) << (8 * j);
}
template <typename Word>
__device__ __forceinline__ int QUnpack(Word word, int j) {
    return static_cast<int8_t>((word >> (8 * j)) & 0xff);
}
// dequantized sum of byte j of two packed words
__device__ __forceinline__ float QSum(int32_t a, float as, int32_t b, float bs, int j) {
    return QUnpack(a, j) * as + QUnpack(b, j) * bs;
}
// W quantized values at payload[i]: one word for W == 4, one byte for W == 1
template <int W>
__device__ __forceinline__ int32_t QLoad(const int8_t* payload, size_t i) {
    if constexpr (W == 4) return reinterpret_cast<const int32_t*>(payload)[i >> 2];
    else return payload[i];
}
template <int W>
__device__ __forceinline__ void QStore(int8_t* payload, size_t i, uint32_t word) {
    if constexpr (W == 4) reinterpret_cast<uint32_t*>(payload)[i >> 2] = word;
    else payload[i] = static_cast<int8_t>(word);
}

__device__ __forceinline__ float WireScale(const uint8_t* wblock) {
    return reinterpret_cast<const float*>(wblock)[0];
}
__device__ __forceinline__ void WriteWireHeader(uint8_t* wblock, float scale) {
    float* hdr = reinterpret_cast<float*>(wblock);
    hdr[0] = scale;
    hdr[1] = 0.f;
}

// Wave-per-block kernels: each 64-lane wavefront owns one wire block (4
// waves per 256-thread workgroup, grid-strided over blocks). The scale
// reduction is a pure cross-lane shuffle — no LDS, no __syncthreads — so
// small blocks stay launch- and HBM-bound, not barrier-bound.
__device__ __forceinline__ float WaveMax(float m) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        m = fmaxf(m, __shfl_down(m, off, 64));
    return __shfl(m, 0, 64);
}

// Half-wave (32-lane) max: __shfl_xor with width 32 stays inside each half.
__device__ __forceinline__ float HalfWaveMax(float m) {
#pragma unroll
    for (int off = 16; off > 0; off >>= 1)
        m = fmaxf(m, __shfl_xor(m, off, 32));
    return m;
}

// f(blk, lane) for every block this wave owns. The grid position comes in
// as default arguments so that it is read in the calling __global__
// function: only there do blockDim/gridDim fold to scalar kernarg loads.
template <typename F>
__device__ __forceinline__ void ForEachWaveBlock(
    size_t nblocks, F f, size_t gtid = blockIdx.x * blockDim.x + threadIdx.x,
    size_t gthreads = gridDim.x * blockDim.x) {
    const int lane = threadIdx.x & 63;
    for (size_t blk = gtid >> 6; blk < nblocks; blk += gthreads >> 6) f(blk, lane);
}

// f(blk, sub) with one wave owning TWO blocks, one per 32-lane half; sub is
// the lane's index inside its half. The last pair's second half idles when
// nblocks is odd.
template <typename F>
__device__ __forceinline__ void ForEachHalfWaveBlock(
    size_t nblocks, F f, size_t gtid = blockIdx.x * blockDim.x + threadIdx.x,
    size_t gthreads = gridDim.x * blockDim.x) {
    ForEachWaveBlock(
        (nblocks + 1) / 2,
        [&](size_t pair, int lane) {
            const size_t blk = pair * 2 + (lane >> 5);
            if (blk < nblocks) f(blk, lane & 31);
        },
        gtid, gthreads);
}

// f(i, width) over the n elements of one block: 4 consecutive elements per
// lane at stride 256 plus a lane-strided tail of single elements when vec4,
// else single elements throughout. width arrives as an integral_constant.
template <typename F>
__device__ __forceinline__ void ForEachBlockElem(size_t n, bool vec4, int lane, F f) {
    using One = std::integral_constant<int, 1>;
    if (vec4) {
        for (size_t i = lane * 4; i + 3 < n; i += 256)
            f(i, std::integral_constant<int, 4>{});
        for (size_t i = (n & ~size_t(3)) + lane; i < n; i += 64) f(i, One{});
    } else {
        for (size_t i = lane; i < n; i += 64) f(i, One{});
    }
}

template <typename T, bool USE_ERR>
__global__ void QuantizeKernel(const T* __restrict__ in, T* __restrict__ err,
                               uint8_t* __restrict__ wire, size_t count,
                               size_t block_elems) {
    const bool vec4 = (block_elems & 3) == 0;
    ForEachWaveBlock((count + block_elems - 1) / block_elems, [&](size_t blk, int lane) {
        const size_t base = blk * block_elems;
        const size_t n = min(block_elems, count - base);
        uint8_t* wblock = wire + blk * (block_elems + kWireHdr);
        int8_t* payload = reinterpret_cast<int8_t*>(wblock + kWireHdr);
        auto value = [&](size_t i) {
            float v = Decode(in[base + i]);
            if (USE_ERR) v += Decode(err[base + i]);
            return v;
        };

        float m = 0.f;
        ForEachBlockElem(n, vec4, lane, [&](size_t i, auto w) {
#pragma unroll
            for (int j = 0; j < decltype(w)::value; ++j)
                m = fmaxf(m, fabsf(value(i + j)));
        });
        const float scale = QScale(WaveMax(m));
        if (lane == 0) WriteWireHeader(wblock, scale);
        const float inv = 1.f / scale;
        ForEachBlockElem(n, vec4, lane, [&](size_t i, auto w) {
            constexpr int W = decltype(w)::value;
            uint32_t packed = 0;
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const float v = value(i + j);
                const float q = QRound(v, inv);
                packed |= QPack(q, j);
                if (USE_ERR) err[base + i + j] = Encode<T>(v - q * scale);
            }
            QStore<W>(payload, i, packed);
        });
        for (size_t i = n + lane; i < block_elems; i += 64) payload[i] = 0;
    });
}

template <typename T, bool NT = false>
__global__ void DequantizeKernel(const uint8_t* __restrict__ wire, T* __restrict__ out,
                                 size_t count, size_t block_elems) {
    // 16-B stores need a 16-B-aligned output base (sliced tensors may not be)
    const bool vec4 = (block_elems & 3) == 0 &&
                      (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    ForEachWaveBlock((count + block_elems - 1) / block_elems, [&](size_t blk, int lane) {
        const size_t base = blk * block_elems;
        const size_t n = min(block_elems, count - base);
        const uint8_t* wblock = wire + blk * (block_elems + kWireHdr);
        const float scale = WireScale(wblock);
        const int8_t* payload = reinterpret_cast<const int8_t*>(wblock + kWireHdr);
        ForEachBlockElem(n, vec4, lane, [&](size_t i, auto w) {
            constexpr int W = decltype(w)::value;
            const int32_t packed =
                NT && W == 4 ? __builtin_nontemporal_load(
                                   reinterpret_cast<const int32_t*>(payload) + (i >> 2))
                             : QLoad<W>(payload, i);
            if constexpr (W == 4 && sizeof(T) == 4) {
                // f32: one 16-B store per lane pass
                float4_ev v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = QUnpack(packed, j) * scale;
                float4_ev* dst4 = reinterpret_cast<float4_ev*>(out + base + i);
                if constexpr (NT) __builtin_nontemporal_store(v, dst4);
                else *dst4 = v;
            } else {
#pragma unroll
                for (int j = 0; j < W; ++j)
                    out[base + i + j] = Encode<T>(QUnpack(packed, j) * scale);
            }
        });
    });
}

// Eight consecutive elements per lane as floats: one 16-B access for bf16,
// two for f32. The only per-type part of the two-blocks-per-wave kernels.
__device__ __forceinline__ void Load8(const unsigned short* p, float v[8]) {
    const ushort8_t a = *reinterpret_cast<const ushort8_t*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = Decode(a[j]);
}
__device__ __forceinline__ void Load8(const float* p, float v[8]) {
    const float4_ev a0 = *reinterpret_cast<const float4_ev*>(p);
    const float4_ev a1 = *reinterpret_cast<const float4_ev*>(p + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = a0[j]; v[4 + j] = a1[j]; }
}
template <bool NT, typename V>
__device__ __forceinline__ void StoreVec(V v, void* p) {
    if constexpr (NT) __builtin_nontemporal_store(v, static_cast<V*>(p));
    else *static_cast<V*>(p) = v;
}
template <bool NT>
__device__ __forceinline__ void Store8(unsigned short* p, const float v[8]) {
    ushort8_t r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = Encode<unsigned short>(v[j]);
    StoreVec<NT>(r, p);
}
template <bool NT>
__device__ __forceinline__ void Store8(float* p, const float v[8]) {
    StoreVec<NT>(float4_ev{v[0], v[1], v[2], v[3]}, p);
    StoreVec<NT>(float4_ev{v[4], v[5], v[6], v[7]}, p + 4);
}

// Fast path (block_elems == 256, whole blocks): one 64-lane wave owns TWO
// wire blocks — each 32-lane half owns one block at 8 elements per lane,
// doubling the per-lane access width and ILP over the generic path. Scale
// reduction is a half-wave shuffle; measured A/B against the generic kernel
// in docs/BENCHMARKS.md. NT_ST stores wire and err nontemporally (A/B hook).
template <typename T, bool USE_ERR, bool NT_ST>
__global__ void QuantizeX2Kernel(const T* __restrict__ in, T* __restrict__ err,
                                 uint8_t* __restrict__ wire, size_t nblocks) {
    ForEachHalfWaveBlock(nblocks, [&](size_t blk, int sub) {
        const size_t base = blk * kFastBlock + sub * 8;
        float v[8];
        Load8(in + base, v);
        if (USE_ERR) {
            float e[8];
            Load8(err + base, e);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] += e[j];
        }
        float m = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(v[j]));
        const float scale = QScale(HalfWaveMax(m));
        const float inv = 1.f / scale;
        uint8_t* wblock = wire + blk * (kFastBlock + kWireHdr);
        if (sub == 0) WriteWireHeader(wblock, scale);
        uint2_ev packed{0, 0};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float q = QRound(v[j], inv);
            packed[j >> 2] |= QPack(q, j & 3);
            v[j] -= q * scale;  // residual, stored only with USE_ERR
        }
        StoreVec<NT_ST>(packed, wblock + kWireHdr + sub * 8);
        if (USE_ERR) Store8<NT_ST>(err + base, v);
    });
}

__global__ void DequantizeBf16x2Kernel(const uint8_t* __restrict__ wire,
                                       unsigned short* __restrict__ out,
                                       size_t nblocks) {
    ForEachHalfWaveBlock(nblocks, [&](size_t blk, int sub) {
        const uint8_t* wblock = wire + blk * (kFastBlock + kWireHdr);
        const float scale = WireScale(wblock);
        const uint2_ev packed =
            *reinterpret_cast<const uint2_ev*>(wblock + kWireHdr + sub * 8);
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = QUnpack(packed[j >> 2], j & 3) * scale;
        Store8<false>(out + blk * kFastBlock + sub * 8, o);
    });
}

__global__ void DequantizeF32x2Kernel(const uint8_t* __restrict__ wire,
                                      float* __restrict__ out, size_t nblocks) {
    ForEachHalfWaveBlock(nblocks, [&](size_t blk, int sub) {
        const uint8_t* wblock = wire + blk * (kFastBlock + kWireHdr);
        const float scale = WireScale(wblock);
        // Split-half layout: lane handles elems [sub*4, +3] and
        // [128 + sub*4, +3] — each of the two 16-B stores is contiguous
        // across the 32 lanes (PMC showed the interleaved 32-B-stride
        // variant emitting +15% write traffic from split cache lines).
        const uint32_t* p4 = reinterpret_cast<const uint32_t*>(wblock + kWireHdr);
        const uint32_t pk0 = __builtin_nontemporal_load(p4 + sub);
        const uint32_t pk1 = __builtin_nontemporal_load(p4 + 32 + sub);
        float4_ev o0, o1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            o0[j] = QUnpack(pk0, j) * scale;
            o1[j] = QUnpack(pk1, j) * scale;
        }
        float* obase = out + blk * kFastBlock;
        StoreVec<true>(o0, obase + sub * 4);
        StoreVec<true>(o1, obase + 128 + sub * 4);
    });
}

// acc_wire += wire in the compressed domain: dequant both, sum, requant with
// a fresh scale (the reference's external reduce_sum hook, quant/quant.c:89).
//
// Fast path (block_elems == 256, full block): one wave owns one block and
// each lane owns exactly 4 elements, so the dequantized sums live in
// registers across the max-reduce and the requant — one load pair, one
// store, half the VALU of the generic two-pass version below.
__global__ void QuantAccum256Kernel(uint8_t* __restrict__ acc,
                                    const uint8_t* __restrict__ in,
                                    size_t nblocks) {
    ForEachWaveBlock(nblocks, [&](size_t blk, int lane) {
        uint8_t* ablock = acc + blk * (kFastBlock + kWireHdr);
        const uint8_t* iblock = in + blk * (kFastBlock + kWireHdr);
        const float as = WireScale(ablock), is = WireScale(iblock);
        int8_t* ap = reinterpret_cast<int8_t*>(ablock + kWireHdr);
        const int32_t pa = QLoad<4>(ap, lane * 4);
        const int32_t pb =
            QLoad<4>(reinterpret_cast<const int8_t*>(iblock + kWireHdr), lane * 4);
        float v[4];
        float m = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = QSum(pa, as, pb, is, j);
            m = fmaxf(m, fabsf(v[j]));
        }
        const float ns = QScale(WaveMax(m));
        const float inv = 1.f / ns;
        uint32_t packed = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) packed |= QPack(QRound(v[j], inv), j);
        QStore<4>(ap, lane * 4, packed);
        if (lane == 0) reinterpret_cast<float*>(ablock)[0] = ns;
    });
}

__device__ __forceinline__ void QuantAccumBody(uint8_t* __restrict__ acc,
                                               const uint8_t* __restrict__ in,
                                               size_t count, size_t block_elems) {
    const bool vec4 = (block_elems & 3) == 0;
    ForEachWaveBlock((count + block_elems - 1) / block_elems, [&](size_t blk, int lane) {
        const size_t n = min(block_elems, count - blk * block_elems);
        uint8_t* ablock = acc + blk * (block_elems + kWireHdr);
        const uint8_t* iblock = in + blk * (block_elems + kWireHdr);
        const float as = WireScale(ablock), is = WireScale(iblock);
        int8_t* ap = reinterpret_cast<int8_t*>(ablock + kWireHdr);
        const int8_t* ip = reinterpret_cast<const int8_t*>(iblock + kWireHdr);

        float m = 0.f;
        ForEachBlockElem(n, vec4, lane, [&](size_t i, auto w) {
            constexpr int W = decltype(w)::value;
            const int32_t pa = QLoad<W>(ap, i), pb = QLoad<W>(ip, i);
#pragma unroll
            for (int j = 0; j < W; ++j) m = fmaxf(m, fabsf(QSum(pa, as, pb, is, j)));
        });
        const float ns = QScale(WaveMax(m));
        const float inv = 1.f / ns;
        ForEachBlockElem(n, vec4, lane, [&](size_t i, auto w) {
            constexpr int W = decltype(w)::value;
            const int32_t pa = QLoad<W>(ap, i), pb = QLoad<W>(ip, i);
            uint32_t packed = 0;
#pragma unroll
            for (int j = 0; j < W; ++j)
                packed |= QPack(QRound(QSum(pa, as, pb, is, j), inv), j);
            QStore<W>(ap, i, packed);
        });
        if (lane == 0) reinterpret_cast<float*>(ablock)[0] = ns;
    });
}

__global__ void QuantAccumKernel(uint8_t* __restrict__ acc,
                                 const uint8_t* __restrict__ in, size_t count,
                                 size_t block_elems) {
    QuantAccumBody(acc, in, count, block_elems);
}

// out = dequant(a) + dequant(b) in the element type: the last hop of the
// quantized reduce-scatter. The sum is never requantized, so the final rank
// saves one lossy step and one pass over the wire (accumulate + dequantize).
// Both wires are local by now (the arrived one was copied out of its
// hand-off slot), so plain loads. Stores are plain here; the fast path below
// turns nontemporal for outputs too large to stay cached.
template <typename T>
__global__ void QuantSumDequantKernel(const uint8_t* __restrict__ a,
                                      const uint8_t* __restrict__ b,
                                      T* __restrict__ out, size_t count,
                                      size_t block_elems) {
    // 16-B (f32) / 8-B (bf16) stores need a 16-B-aligned output base
    const bool vec4 = (block_elems & 3) == 0 &&
                      (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    ForEachWaveBlock((count + block_elems - 1) / block_elems, [&](size_t blk, int lane) {
        const size_t base = blk * block_elems;
        const size_t n = min(block_elems, count - base);
        const uint8_t* ablock = a + blk * (block_elems + kWireHdr);
        const uint8_t* bblock = b + blk * (block_elems + kWireHdr);
        const float as = WireScale(ablock), bs = WireScale(bblock);
        const int8_t* ap = reinterpret_cast<const int8_t*>(ablock + kWireHdr);
        const int8_t* bp = reinterpret_cast<const int8_t*>(bblock + kWireHdr);
        ForEachBlockElem(n, vec4, lane, [&](size_t i, auto w) {
            constexpr int W = decltype(w)::value;
            const int32_t pa = QLoad<W>(ap, i), pb = QLoad<W>(bp, i);
            if constexpr (W == 4) {
                std::conditional_t<sizeof(T) == 4, float4_ev, ushort4_t> v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = Encode<T>(QSum(pa, as, pb, bs, j));
                StoreVec<false>(v, out + base + i);
            } else {
                out[base + i] = Encode<T>(QSum(pa, as, pb, bs, 0));
            }
        });
    });
}

// Fast path (block_elems == 256, whole blocks): two blocks per wave as in
// the dequantize kernels. bf16 takes 8 consecutive elements per lane (one
// 16-B store); f32 takes the split-half layout of DequantizeF32x2Kernel so
// that each of its two 16-B stores is contiguous across the half-wave.
// NT_ST stores `out` nontemporally (size rule and A/B in the launcher).
template <typename T, bool NT_ST>
__global__ void QuantSumDequantX2Kernel(const uint8_t* __restrict__ a,
                                        const uint8_t* __restrict__ b,
                                        T* __restrict__ out, size_t nblocks) {
    ForEachHalfWaveBlock(nblocks, [&](size_t blk, int sub) {
        const uint8_t* ablock = a + blk * (kFastBlock + kWireHdr);
        const uint8_t* bblock = b + blk * (kFastBlock + kWireHdr);
        const float as = WireScale(ablock), bs = WireScale(bblock);
        T* obase = out + blk * kFastBlock;
        float o[8];
        if constexpr (sizeof(T) == 4) {
            const int32_t* a4 = reinterpret_cast<const int32_t*>(ablock + kWireHdr);
            const int32_t* b4 = reinterpret_cast<const int32_t*>(bblock + kWireHdr);
            const int32_t pa0 = a4[sub], pa1 = a4[32 + sub];
            const int32_t pb0 = b4[sub], pb1 = b4[32 + sub];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                o[j] = QSum(pa0, as, pb0, bs, j);
                o[4 + j] = QSum(pa1, as, pb1, bs, j);
            }
            StoreVec<NT_ST>(float4_ev{o[0], o[1], o[2], o[3]}, obase + sub * 4);
            StoreVec<NT_ST>(float4_ev{o[4], o[5], o[6], o[7]}, obase + 128 + sub * 4);
        } else {
            const uint2_ev pa =
                *reinterpret_cast<const uint2_ev*>(ablock + kWireHdr + sub * 8);
            const uint2_ev pb =
                *reinterpret_cast<const uint2_ev*>(bblock + kWireHdr + sub * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                o[j] = QSum(static_cast<int32_t>(pa[j >> 2]), as,
                            static_cast<int32_t>(pb[j >> 2]), bs, j & 3);
            Store8<NT_ST>(obase + sub * 8, o);
        }
    });
}

// N-way fan-in of the one-shot quantized reduce-scatter: out = the sum of NW
// dequantized wires, each quantized once and none requantized. The wire
// pointers travel by value in the kernarg (as FanKernArgs does), so they are
// scalar loads and no table has to live in device memory.
constexpr int kMaxSumWires = 8;
struct QuantWires {
    const uint8_t* w[kMaxSumWires];
};

// Byte j of each wire's packed word, summed in wire order from +0 with one
// explicit fma per wire: the result is a fixed function of the wires that no
// contraction setting can change (a*b + c*d may or may not be fused).
template <int NW>
__device__ __forceinline__ float QFmaSum(const int32_t (&p)[NW], const float (&s)[NW],
                                         int j) {
    float acc = 0.f;
#pragma unroll
    for (int r = 0; r < NW; ++r)
        acc = __builtin_fmaf(static_cast<float>(QUnpack(p[r], j)), s[r], acc);
    return acc;
}

// Generic path: any legal block, partial last block, unaligned `out`. All NW
// loads of a pass are issued before the first fma, so they are in flight
// together.
template <typename T, int NW>
__global__ void QuantSumDequantNKernel(QuantWires ws, T* __restrict__ out, size_t count,
                                       size_t block_elems) {
    const bool vec4 = (block_elems & 3) == 0 &&
                      (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    ForEachWaveBlock((count + block_elems - 1) / block_elems, [&](size_t vblk, int lane) {
        // The block index is the same in all 64 lanes; saying so keeps the
        // NW block addresses in scalar registers (with 8 wires they spilled
        // as per-lane values).
        const size_t blk =
            (static_cast<size_t>(__builtin_amdgcn_readfirstlane(
                 static_cast<uint32_t>(vblk >> 32))) << 32) |
            static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(vblk)));
        const size_t base = blk * block_elems;
        const size_t n = min(block_elems, count - base);
        const int8_t* payload[NW];
        float s[NW];
#pragma unroll
        for (int r = 0; r < NW; ++r) {
            const uint8_t* wblock = ws.w[r] + blk * (block_elems + kWireHdr);
            s[r] = WireScale(wblock);
            payload[r] = reinterpret_cast<const int8_t*>(wblock + kWireHdr);
        }
        ForEachBlockElem(n, vec4, lane, [&](size_t i, auto w) {
            constexpr int W = decltype(w)::value;
            int32_t p[NW];
#pragma unroll
            for (int r = 0; r < NW; ++r) p[r] = QLoad<W>(payload[r], i);
            if constexpr (W == 4) {
                std::conditional_t<sizeof(T) == 4, float4_ev, ushort4_t> v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = Encode<T>(QFmaSum<NW>(p, s, j));
                StoreVec<false>(v, out + base + i);
            } else {
                out[base + i] = Encode<T>(QFmaSum<NW>(p, s, 0));
            }
        });
    });
}

// Fast path (block_elems == 256, whole blocks, 16-B aligned `out`): one
// block per half-wave, 8 consecutive elements per lane, so each wire costs a
// lane one 8-B payload load (wires are only 8-B aligned) and the output one
// 16-B store for bf16, two for f32.
template <typename T, int NW>
__global__ void QuantSumDequantNX2Kernel(QuantWires ws, T* __restrict__ out,
                                         size_t nblocks) {
    ForEachHalfWaveBlock(nblocks, [&](size_t blk, int sub) {
        uint2_ev pw[NW];
        float s[NW];
#pragma unroll
        for (int r = 0; r < NW; ++r) {
            const uint8_t* wblock = ws.w[r] + blk * (kFastBlock + kWireHdr);
            s[r] = WireScale(wblock);
            pw[r] = *reinterpret_cast<const uint2_ev*>(wblock + kWireHdr + sub * 8);
        }
        float o[8];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            int32_t p[NW];
#pragma unroll
            for (int r = 0; r < NW; ++r) p[r] = static_cast<int32_t>(pw[r][h]);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[4 * h + j] = QFmaSum<NW>(p, s, j);
        }
        Store8<false>(out + blk * kFastBlock + sub * 8, o);
    });
}

// The owner's step of the two-shot quantized allreduce: dst = requantize(sum
// of NW dequantized wires), over whole wire units. The sum is QFmaSum, the
// requantize is QuantizeKernel's (QScale, 1/scale, QRound, QPack,
// WriteWireHeader). `dst` may be exactly one of the wires, so neither side is
// __restrict__: a lane stores only payload bytes it has itself loaded, and the
// header is stored after the cross-lane maximum, which needs every lane's
// scale loads. Plain stores: the destination is sent to peers next.
//
// Generic path: any legal block, one wave per unit, two passes. The second
// pass recomputes the fma chain instead of holding a block in registers.
template <int NW>
__global__ void QuantSumRequantNKernel(QuantWires ws, uint8_t* dst, size_t nunits,
                                       size_t block_elems) {
    ForEachWaveBlock(nunits, [&](size_t vblk, int lane) {
        // scalar block index, as in QuantSumDequantNKernel
        const size_t blk =
            (static_cast<size_t>(__builtin_amdgcn_readfirstlane(
                 static_cast<uint32_t>(vblk >> 32))) << 32) |
            static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(vblk)));
        const int8_t* payload[NW];
        float s[NW];
#pragma unroll
        for (int r = 0; r < NW; ++r) {
            const uint8_t* wblock = ws.w[r] + blk * (block_elems + kWireHdr);
            s[r] = WireScale(wblock);
            payload[r] = reinterpret_cast<const int8_t*>(wblock + kWireHdr);
        }
        uint8_t* dblock = dst + blk * (block_elems + kWireHdr);
        int8_t* dpayload = reinterpret_cast<int8_t*>(dblock + kWireHdr);

        float m = 0.f;
        ForEachBlockElem(block_elems, true, lane, [&](size_t i, auto w) {
            constexpr int W = decltype(w)::value;
            int32_t p[NW];
#pragma unroll
            for (int r = 0; r < NW; ++r) p[r] = QLoad<W>(payload[r], i);
#pragma unroll
            for (int j = 0; j < W; ++j) m = fmaxf(m, fabsf(QFmaSum<NW>(p, s, j)));
        });
        const float scale = QScale(WaveMax(m));
        const float inv = 1.f / scale;
        ForEachBlockElem(block_elems, true, lane, [&](size_t i, auto w) {
            constexpr int W = decltype(w)::value;
            int32_t p[NW];
#pragma unroll
            for (int r = 0; r < NW; ++r) p[r] = QLoad<W>(payload[r], i);
            uint32_t packed = 0;
#pragma unroll
            for (int j = 0; j < W; ++j) packed |= QPack(QRound(QFmaSum<NW>(p, s, j), inv), j);
            QStore<W>(dpayload, i, packed);
        });
        if (lane == 0) WriteWireHeader(dblock, scale);
    });
}

// Fast path (block_elems == 256, 8-B aligned wires and dst): one unit per
// half-wave, the 8 sums of a lane live in registers across the half-wave
// maximum, so each wire costs a lane one 8-B payload load and the result one
// 8-B payload store.
template <int NW>
__global__ void QuantSumRequantNX2Kernel(QuantWires ws, uint8_t* dst, size_t nunits) {
    ForEachHalfWaveBlock(nunits, [&](size_t blk, int sub) {
        uint2_ev pw[NW];
        float s[NW];
#pragma unroll
        for (int r = 0; r < NW; ++r) {
            const uint8_t* wblock = ws.w[r] + blk * (kFastBlock + kWireHdr);
            s[r] = WireScale(wblock);
            pw[r] = *reinterpret_cast<const uint2_ev*>(wblock + kWireHdr + sub * 8);
        }
        float v[8];
        float m = 0.f;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            int32_t p[NW];
#pragma unroll
            for (int r = 0; r < NW; ++r) p[r] = static_cast<int32_t>(pw[r][h]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[4 * h + j] = QFmaSum<NW>(p, s, j);
                m = fmaxf(m, fabsf(v[4 * h + j]));
            }
        }
        const float scale = QScale(HalfWaveMax(m));
        const float inv = 1.f / scale;
        uint2_ev packed{0, 0};
#pragma unroll
        for (int j = 0; j < 8; ++j) packed[j >> 2] |= QPack(QRound(v[j], inv), j & 3);
        uint8_t* dblock = dst + blk * (kFastBlock + kWireHdr);
        StoreVec<false>(packed, dblock + kWireHdr + sub * 8);
        if (sub == 0) WriteWireHeader(dblock, scale);
    });
}

inline size_t NumBlocks(size_t count, size_t block_elems) {
    return (count + block_elems - 1) / block_elems;
}
// 4 waves per 256-thread workgroup, grid-strided over wire blocks.
inline dim3 WaveGrid(size_t nblocks) {
    return dim3(static_cast<uint32_t>(std::min<size_t>((nblocks + 3) / 4, kMaxGrid)));
}
inline dim3 PairGrid(size_t nblocks) { return WaveGrid((nblocks + 1) / 2); }

// Two-blocks-per-wave fast path: whole 256-element blocks, 16-B aligned
// element buffers (`err` may be null), 8-B aligned wire; f32 only from
// 4 MiB up (below that the generic kernel wins).
bool X2Eligible(size_t count, size_t block_elems, DataType dt, const void* elems,
                const void* err, const void* wire) {
    return block_elems == kFastBlock && count % kFastBlock == 0 &&
           (dt != DataType::F32 || count * 4 >= (4u << 20)) &&
           ((reinterpret_cast<uintptr_t>(elems) | reinterpret_cast<uintptr_t>(err)) & 15) == 0 &&
           (reinterpret_cast<uintptr_t>(wire) & 7) == 0;
}

template <typename T>
void QuantizeTyped(const void* in, void* err, void* wire, size_t count,
                   size_t block_elems, DataType dt, bool use_err, hipStream_t stream) {
    const size_t nblocks = NumBlocks(count, block_elems);
    const T* i = static_cast<const T*>(in);
    T* e = static_cast<T*>(err);
    uint8_t* w = static_cast<uint8_t*>(wire);
    DispatchBool(use_err, [&](auto ue) {
        constexpr bool UE = decltype(ue)::value;
        if (X2Eligible(count, block_elems, dt, in, err, wire))
            QuantizeX2Kernel<T, UE, false><<<PairGrid(nblocks), dim3(kBlock), 0, stream>>>(
                i, e, w, nblocks);
        else
            QuantizeKernel<T, UE><<<WaveGrid(nblocks), dim3(kBlock), 0, stream>>>(
                i, e, w, count, block_elems);
    });
}

template <typename T, bool NT>
void DequantizeGeneric(const void* wire, void* out, size_t count, size_t block_elems,
                       hipStream_t stream) {
    DequantizeKernel<T, NT><<<WaveGrid(NumBlocks(count, block_elems)), dim3(kBlock), 0, stream>>>(
        static_cast<const uint8_t*>(wire), static_cast<T*>(out), count, block_elems);
}

}  // namespace

void LaunchQuantize(const void* in, void* err, void* wire, size_t count,
                    size_t block_elems, DataType dt, bool use_err,
                    hipStream_t stream) {
    CheckQuantBlock(block_elems, "LaunchQuantize");
    if (dt == DataType::F32)
        QuantizeTyped<float>(in, err, wire, count, block_elems, dt, use_err, stream);
    else if (dt == DataType::BF16)
        QuantizeTyped<unsigned short>(in, err, wire, count, block_elems, dt, use_err, stream);
    else
        MLSL_THROW("quantization supports f32/bf16 only");
    HIP_CHECK(hipGetLastError());
}

void LaunchDequantize(const void* wire, void* out, size_t count,
                      size_t block_elems, DataType dt, hipStream_t stream) {
    CheckQuantBlock(block_elems, "LaunchDequantize");
    const bool x2 = X2Eligible(count, block_elems, dt, out, nullptr, wire);
    const size_t nblocks = NumBlocks(count, block_elems);
    const uint8_t* w = static_cast<const uint8_t*>(wire);
    if (dt == DataType::F32) {
        // NT past L2 reach: measured 3.00 -> 3.17 TB/s effective at 256 MiB
        // (stream-once wire + output); small outputs keep L2 retention for
        // the consumer.
        if (x2)
            DequantizeF32x2Kernel<<<PairGrid(nblocks), dim3(kBlock), 0, stream>>>(
                w, static_cast<float*>(out), nblocks);
        else if (count * sizeof(float) >= (16u << 20))
            DequantizeGeneric<float, true>(wire, out, count, block_elems, stream);
        else
            DequantizeGeneric<float, false>(wire, out, count, block_elems, stream);
    } else if (dt == DataType::BF16) {
        if (x2)
            DequantizeBf16x2Kernel<<<PairGrid(nblocks), dim3(kBlock), 0, stream>>>(
                w, static_cast<unsigned short*>(out), nblocks);
        else
            DequantizeGeneric<unsigned short, false>(wire, out, count, block_elems, stream);
    } else {
        MLSL_THROW("dequantization supports f32/bf16 only");
    }
    HIP_CHECK(hipGetLastError());
}

void LaunchQuantizeF32NT(const void* in, void* err, void* wire, size_t count,
                         size_t block_elems, hipStream_t stream) {
    // A/B hook: f32 two-blocks-per-wave with NT stores for wire+err.
    MLSL_CHECK(block_elems == kFastBlock && count % kFastBlock == 0,
               "NT A/B needs whole 256-blocks");
    const size_t nblocks = count / kFastBlock;
    QuantizeX2Kernel<float, true, true><<<PairGrid(nblocks), dim3(kBlock), 0, stream>>>(
        static_cast<const float*>(in), static_cast<float*>(err),
        static_cast<uint8_t*>(wire), nblocks);
    HIP_CHECK(hipGetLastError());
}

void LaunchDequantizeNT(const void* wire, void* out, size_t count,
                        size_t block_elems, DataType dt, hipStream_t stream) {
    CheckQuantBlock(block_elems, "LaunchDequantizeNT");
    // f32-only NT variant (A/B benchmark hook): stream-once wire reads and
    // output stores skip L2 retention.
    if (dt != DataType::F32) {
        LaunchDequantize(wire, out, count, block_elems, dt, stream);
        return;
    }
    DequantizeGeneric<float, true>(wire, out, count, block_elems, stream);
    HIP_CHECK(hipGetLastError());
}

void LaunchQuantAccum(void* acc_wire, const void* wire, size_t count,
                      size_t block_elems, hipStream_t stream) {
    CheckQuantBlock(block_elems, "LaunchQuantAccum");
    if (count == 0) return;
    const size_t nblocks = NumBlocks(count, block_elems);
    uint8_t* a = static_cast<uint8_t*>(acc_wire);
    const uint8_t* w = static_cast<const uint8_t*>(wire);
    if (block_elems == kFastBlock && count % kFastBlock == 0)
        QuantAccum256Kernel<<<WaveGrid(nblocks), dim3(kBlock), 0, stream>>>(a, w, nblocks);
    else
        QuantAccumKernel<<<WaveGrid(nblocks), dim3(kBlock), 0, stream>>>(a, w, count,
                                                                         block_elems);
    HIP_CHECK(hipGetLastError());
}

namespace {

// Wires sit at multiples of the 264-B wire block inside a request's scratch
// (TMP slots, per-rank segments), so they are only 8-B aligned, like the
// wire of X2Eligible. No size floor: the epilogue has no slower-start
// generic sibling to beat at small sizes.
bool SumDequantX2Eligible(size_t count, size_t block_elems, const void* a,
                          const void* b, const void* out) {
    return block_elems == kFastBlock && count % kFastBlock == 0 &&
           (reinterpret_cast<uintptr_t>(out) & 15) == 0 &&
           ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 7) == 0;
}

// Nontemporal stores of `out` from 128 MiB up: measured 95.6 -> 81.9 us at
// 256 MiB (f32) and 62.9 -> 60.0 us at 128 MiB (bf16); at 64 MiB and below
// the gain is 0-3 % (docs/BENCHMARKS.md), and plain stores leave a gradient
// shard of that size in cache for the optimizer that reads it next.
constexpr size_t kSumDequantNtBytes = size_t(128) << 20;

template <typename T>
void QuantSumDequantTyped(const void* a_wire, const void* b_wire, void* out,
                          size_t count, size_t block_elems, bool force_nt,
                          hipStream_t stream) {
    const size_t nblocks = NumBlocks(count, block_elems);
    const uint8_t* a = static_cast<const uint8_t*>(a_wire);
    const uint8_t* b = static_cast<const uint8_t*>(b_wire);
    if (SumDequantX2Eligible(count, block_elems, a_wire, b_wire, out))
        DispatchBool(force_nt || count * sizeof(T) >= kSumDequantNtBytes, [&](auto nt) {
            QuantSumDequantX2Kernel<T, decltype(nt)::value>
                <<<PairGrid(nblocks), dim3(kBlock), 0, stream>>>(
                    a, b, static_cast<T*>(out), nblocks);
        });
    else
        QuantSumDequantKernel<T><<<WaveGrid(nblocks), dim3(kBlock), 0, stream>>>(
            a, b, static_cast<T*>(out), count, block_elems);
}

void QuantSumDequantAny(const void* a_wire, const void* b_wire, void* out,
                        size_t count, size_t block_elems, DataType dt, bool force_nt,
                        hipStream_t stream, const char* who) {
    CheckQuantBlock(block_elems, who);
    if (dt != DataType::F32 && dt != DataType::BF16)
        MLSL_THROW("quantized sum-dequantize supports f32/bf16 only");
    if (count == 0) return;
    if (dt == DataType::F32)
        QuantSumDequantTyped<float>(a_wire, b_wire, out, count, block_elems, force_nt,
                                    stream);
    else
        QuantSumDequantTyped<unsigned short>(a_wire, b_wire, out, count, block_elems,
                                             force_nt, stream);
    HIP_CHECK(hipGetLastError());
}

}  // namespace

void LaunchQuantSumDequant(const void* a_wire, const void* b_wire, void* out,
                           size_t count, size_t block_elems, DataType dt,
                           hipStream_t stream) {
    QuantSumDequantAny(a_wire, b_wire, out, count, block_elems, dt, /*force_nt=*/false,
                       stream, "LaunchQuantSumDequant");
}

void LaunchQuantSumDequantNT(const void* a_wire, const void* b_wire, void* out,
                             size_t count, size_t block_elems, DataType dt,
                             hipStream_t stream) {
    // A/B hook: the fast path with nontemporal stores of `out` at any size.
    QuantSumDequantAny(a_wire, b_wire, out, count, block_elems, dt, /*force_nt=*/true,
                       stream, "LaunchQuantSumDequantNT");
}

namespace {

// f(integral_constant<int, nwires>) for nwires in [1, kMaxSumWires]
template <typename F>
void DispatchWires(int nwires, F&& f) {
    switch (nwires) {
#define MLSL_WIRES_CASE(N) case N: f(std::integral_constant<int, N>{}); break;
        MLSL_WIRES_CASE(1) MLSL_WIRES_CASE(2) MLSL_WIRES_CASE(3) MLSL_WIRES_CASE(4)
        MLSL_WIRES_CASE(5) MLSL_WIRES_CASE(6) MLSL_WIRES_CASE(7) MLSL_WIRES_CASE(8)
#undef MLSL_WIRES_CASE
        default: MLSL_THROW("quantized sum-dequantize: wire count out of range");
    }
}

template <typename T>
void QuantSumDequantNTyped(const QuantWires& ws, int nwires, bool x2, void* out,
                           size_t count, size_t block_elems, hipStream_t stream) {
    const size_t nblocks = NumBlocks(count, block_elems);
    DispatchWires(nwires, [&](auto nw) {
        constexpr int NW = decltype(nw)::value;
        if (x2)
            QuantSumDequantNX2Kernel<T, NW><<<PairGrid(nblocks), dim3(kBlock), 0, stream>>>(
                ws, static_cast<T*>(out), nblocks);
        else
            QuantSumDequantNKernel<T, NW><<<WaveGrid(nblocks), dim3(kBlock), 0, stream>>>(
                ws, static_cast<T*>(out), count, block_elems);
    });
}

}  // namespace

void LaunchQuantSumDequantN(const void* const* wires, int nwires, void* out, size_t count,
                            size_t block_elems, DataType dt, hipStream_t stream) {
    CheckQuantBlock(block_elems, "LaunchQuantSumDequantN");
    if (dt != DataType::F32 && dt != DataType::BF16)
        MLSL_THROW("quantized sum-dequantize supports f32/bf16 only");
    MLSL_CHECK(nwires >= 1 && nwires <= kMaxSumWires,
               "quantized sum-dequantize takes 1 to 8 wires");
    if (count == 0) return;
    QuantWires ws{};
    // same fast-path rule as SumDequantX2Eligible, over every wire
    bool x2 = block_elems == kFastBlock && count % kFastBlock == 0 &&
              (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    for (int r = 0; r < nwires; ++r) {
        MLSL_CHECK(wires[r] != nullptr, "quantized sum-dequantize: null wire");
        ws.w[r] = static_cast<const uint8_t*>(wires[r]);
        x2 = x2 && (reinterpret_cast<uintptr_t>(wires[r]) & 7) == 0;
    }
    if (dt == DataType::F32)
        QuantSumDequantNTyped<float>(ws, nwires, x2, out, count, block_elems, stream);
    else
        QuantSumDequantNTyped<unsigned short>(ws, nwires, x2, out, count, block_elems,
                                              stream);
    HIP_CHECK(hipGetLastError());
}

// Aliasing contract: dst_wire may be EXACTLY one of `wires` (the two-shot
// allreduce requantizes into the owner's own range in place) or overlap none
// of them; a partial overlap is not supported. The kernels keep it: a lane
// stores only payload bytes it has loaded itself, and a unit's header is
// stored after the unit's cross-lane maximum, which needs all its scale loads.
void LaunchQuantSumRequantN(const void* const* wires, int nwires, void* dst_wire,
                            size_t nunits, size_t block_elems, hipStream_t stream) {
    CheckQuantBlock(block_elems, "LaunchQuantSumRequantN");
    MLSL_CHECK(nwires >= 1 && nwires <= kMaxSumWires,
               "quantized sum-requantize takes 1 to 8 wires");
    MLSL_CHECK(dst_wire != nullptr, "quantized sum-requantize: null destination");
    QuantWires ws{};
    // headers are floats and payloads are read as 4-byte words
    uintptr_t align = reinterpret_cast<uintptr_t>(dst_wire);
    for (int r = 0; r < nwires; ++r) {
        MLSL_CHECK(wires[r] != nullptr, "quantized sum-requantize: null wire");
        ws.w[r] = static_cast<const uint8_t*>(wires[r]);
        align |= reinterpret_cast<uintptr_t>(wires[r]);
    }
    MLSL_CHECK((align & 3) == 0, "quantized sum-requantize: wires must be 4-byte aligned");
    if (nunits == 0) return;
    const bool x2 = block_elems == kFastBlock && (align & 7) == 0;
    uint8_t* dst = static_cast<uint8_t*>(dst_wire);
    DispatchWires(nwires, [&](auto nw) {
        constexpr int NW = decltype(nw)::value;
        if (x2)
            QuantSumRequantNX2Kernel<NW><<<PairGrid(nunits), dim3(kBlock), 0, stream>>>(
                ws, dst, nunits);
        else
            QuantSumRequantNKernel<NW><<<WaveGrid(nunits), dim3(kBlock), 0, stream>>>(
                ws, dst, nunits, block_elems);
    });
    HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// Pack/unpack between [mb][fm][fmSize] layer layout and comm-buffer blocks.

namespace {

template <typename T, bool PACK>
__global__ void PackKernel(const T* __restrict__ src, T* __restrict__ dst,
                           PackBlockDesc d) {
    const size_t total = d.mb_count * d.fm_count * d.fm_size;
    const size_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = gridDim.x * blockDim.x;
    for (size_t i = tid; i < total; i += stride) {
        const size_t k = i % d.fm_size;
        const size_t fm = (i / d.fm_size) % d.fm_count;
        const size_t mb = i / (d.fm_size * d.fm_count);
        const size_t layer_idx =
            ((d.mb_offset + mb) * d.local_fm_count + d.fm_offset + fm) * d.fm_size + k;
        const size_t buf_idx = d.buf_offset + i;
        if (PACK) dst[buf_idx] = src[layer_idx];
        else dst[layer_idx] = src[buf_idx];
    }
}

// Magic-number unsigned division: M = ceil(2^64 / d); for n < 2^32 the
// high half of n*M is exactly floor(n/d) (error term n*e/(d*2^64) < 2^-32).
// Replaces the per-element 64-bit div/mod pair that dominated the naive
// pack kernel (integer division has no hardware unit on CDNA4 — it
// expands to a long instruction sequence).
struct FastDiv {
    uint64_t M;     // ceil(2^64 / d); 0 means d == 1 (identity)
};

inline FastDiv MakeFastDiv(uint32_t d) {
    FastDiv r;
    r.M = d <= 1 ? 0 : (~0ull / d) + 1;
    return r;
}

__device__ __forceinline__ uint32_t FDiv(uint32_t n, FastDiv f) {
    if (f.M == 0) return n;
    return static_cast<uint32_t>(__umul64hi(static_cast<uint64_t>(n), f.M));
}

template <typename T, bool PACK, bool NT = false>
__global__ void PackFastKernel(const T* __restrict__ src, T* __restrict__ dst,
                               PackBlockDesc d, FastDiv dfs, FastDiv dfc,
                               uint32_t total) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = tid; i < total; i += stride) {
        const uint32_t row = FDiv(i, dfs);                    // i / fm_size
        const uint32_t k = i - row * static_cast<uint32_t>(d.fm_size);
        const uint32_t mb = FDiv(row, dfc);                   // row / fm_count
        const uint32_t fm = row - mb * static_cast<uint32_t>(d.fm_count);
        const size_t layer_idx =
            ((d.mb_offset + mb) * d.local_fm_count + d.fm_offset + fm) * d.fm_size + k;
        const size_t buf_idx = d.buf_offset + i;
        const T* s_ = PACK ? src + layer_idx : src + buf_idx;
        T* d_ = PACK ? dst + buf_idx : dst + layer_idx;
        if constexpr (NT) {
            if constexpr (sizeof(T) == 16) {
                // uint4 is a struct type; the NT builtins need an
                // ext-vector-compatible pointee.
                __builtin_nontemporal_store(
                    __builtin_nontemporal_load(reinterpret_cast<const uint4_ev*>(s_)),
                    reinterpret_cast<uint4_ev*>(d_));
            } else {
                __builtin_nontemporal_store(__builtin_nontemporal_load(s_), d_);
            }
        } else {
            *d_ = *s_;
        }
    }
}

// Row-contiguous blocks whose fm rows are 16-byte multiples vectorize to
// uint4 moves (4x fewer instructions; coalescing unchanged).
bool Pack16(const PackBlockDesc& d, size_t es, PackBlockDesc* out) {
    if ((d.fm_size * es) % 16 != 0 || (d.buf_offset * es) % 16 != 0) return false;
    *out = d;
    out->fm_size = d.fm_size * es / 16;
    out->buf_offset = d.buf_offset * es / 16;
    return true;
}

// Launch the magic-div kernel when totals fit 32 bits (any realistic
// activation block), else the size_t-div fallback.
template <typename T, bool PACK>
void LaunchPackTyped(const void* vsrc, void* vdst, const PackBlockDesc& d,
                     hipStream_t stream) {
    const T* src = static_cast<const T*>(vsrc);
    T* dst = static_cast<T*>(vdst);
    const size_t total = d.mb_count * d.fm_count * d.fm_size;
    const int grid = GridFor(total);
    if (total < (1ull << 32) && d.fm_size < (1ull << 32) &&
        d.fm_count < (1ull << 32)) {
        const FastDiv dfs = MakeFastDiv(static_cast<uint32_t>(d.fm_size));
        const FastDiv dfc = MakeFastDiv(static_cast<uint32_t>(d.fm_count));
        DispatchBool(total * sizeof(T) >= (16u << 20), [&](auto nt) {
            PackFastKernel<T, PACK, decltype(nt)::value><<<dim3(grid), dim3(kBlock), 0, stream>>>(
                src, dst, d, dfs, dfc, static_cast<uint32_t>(total));
        });
    } else {
        PackKernel<T, PACK><<<dim3(grid), dim3(kBlock), 0, stream>>>(src, dst, d);
    }
    HIP_CHECK(hipGetLastError());
}

template <bool PACK>
void LaunchPackOrUnpack(const void* src, void* dst, const PackBlockDesc& d,
                        DataType dt, hipStream_t stream) {
    const size_t es = DtypeSize(dt);
    PackBlockDesc d16;
    if (Pack16(d, es, &d16)) {
        LaunchPackTyped<uint4, PACK>(src, dst, d16, stream);
        return;
    }
    switch (es) {
        case 4: LaunchPackTyped<uint32_t, PACK>(src, dst, d, stream); break;
        case 8: LaunchPackTyped<uint64_t, PACK>(src, dst, d, stream); break;
        case 2: LaunchPackTyped<uint16_t, PACK>(src, dst, d, stream); break;
        default: LaunchPackTyped<uint8_t, PACK>(src, dst, d, stream);
    }
}

}  // namespace

void LaunchPack(const void* src, void* dst, const PackBlockDesc& d, DataType dt,
                hipStream_t stream) {
    LaunchPackOrUnpack<true>(src, dst, d, dt, stream);
}

void LaunchUnpack(const void* src, void* dst, const PackBlockDesc& d, DataType dt,
                  hipStream_t stream) {
    LaunchPackOrUnpack<false>(src, dst, d, dt, stream);
}

// ---------------------------------------------------------------------------
// Segmented dequantize: the finish of the quantized all-gather. The wire is
// nseg segment wires one after the other, each NumBlocks(count) blocks on a
// grid of its own, and segment j goes to out[j * count, (j + 1) * count), in
// one launch for any nseg: the work index runs over all nseg * nblocks wire
// blocks, and since the segment wires are contiguous, wire block `idx` sits
// at idx * (block + 8) whatever its segment.
//
// Minimum traffic per element: 1 wire byte (+ 8 per block) in, sizeof(T) out,
// and with ACC another sizeof(T) in. f32: 5.03 B assign, 9.03 B accumulate;
// bf16: 3.03 B and 5.03 B (block 256).

namespace {

// out = q * scale, or with ACC out = fma(q, scale, out): one explicit fma in
// float as QFmaSum does it, rounded once into T.
template <typename T, bool ACC>
__device__ __forceinline__ T DequantElem(int q, float scale, T old) {
    if constexpr (ACC)
        return Encode<T>(__builtin_fmaf(static_cast<float>(q), scale, Decode(old)));
    else
        return Encode<T>(q * scale);
}

// Generic path: any legal block, partial last blocks, any alignment.
template <typename T, bool ACC>
__global__ void DequantizeSegmentsKernel(const uint8_t* __restrict__ wire, T* out,
                                         size_t count, size_t block_elems,
                                         uint32_t nblocks, FastDiv by_nblocks,
                                         uint32_t total) {
    ForEachWaveBlock(total, [&](size_t vidx, int lane) {
        // uniform across the wave: segment, block and both addresses stay in
        // scalar registers (as in QuantSumDequantNKernel)
        const uint32_t idx = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(vidx));
        const uint32_t seg = FDiv(idx, by_nblocks);
        const uint32_t blk = idx - seg * nblocks;
        const size_t base = static_cast<size_t>(blk) * block_elems;
        const size_t n = min(block_elems, count - base);
        const uint8_t* wblock = wire + static_cast<size_t>(idx) * (block_elems + kWireHdr);
        const float scale = WireScale(wblock);
        const int8_t* payload = reinterpret_cast<const int8_t*>(wblock + kWireHdr);
        // Segment j starts j * count elements in: with a count that is no
        // multiple of 16 bytes an aligned `out` has misaligned segments, so
        // the vector width is decided per segment.
        T* o = out + static_cast<size_t>(seg) * count + base;
        const bool vec4 = (block_elems & 3) == 0 &&
                          (reinterpret_cast<uintptr_t>(o - base) & 15) == 0;
        ForEachBlockElem(n, vec4, lane, [&](size_t i, auto w) {
            constexpr int W = decltype(w)::value;
            const int32_t packed = QLoad<W>(payload, i);
            if constexpr (W == 4) {
                using V = std::conditional_t<sizeof(T) == 4, float4_ev, ushort4_t>;
                V v{};
                if constexpr (ACC) v = *reinterpret_cast<const V*>(o + i);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    v[j] = DequantElem<T, ACC>(QUnpack(packed, j), scale, v[j]);
                StoreVec<false>(v, o + i);
            } else {
                o[i] = DequantElem<T, ACC>(QUnpack(packed, 0), scale, ACC ? o[i] : T{});
            }
        });
    });
}

// Fast path (block_elems == 256, whole blocks, 16-B aligned `out`): every
// segment is whole blocks, so wire and output are both flat runs of `nblocks`
// blocks in all. Two blocks per wave; f32 in the split-half layout of
// DequantizeF32x2Kernel (each 16-B access contiguous across the half-wave),
// bf16 eight consecutive elements per lane; with ACC the loads of `out`
// follow the stores' layout. The wire is only 8-B aligned.
template <typename T, bool ACC, bool NT_ST>
__global__ void DequantizeSegmentsX2Kernel(const uint8_t* __restrict__ wire, T* out,
                                           size_t nblocks) {
    ForEachHalfWaveBlock(nblocks, [&](size_t blk, int sub) {
        const uint8_t* wblock = wire + blk * (kFastBlock + kWireHdr);
        const float scale = WireScale(wblock);
        T* obase = out + blk * kFastBlock;
        if constexpr (sizeof(T) == 4) {
            const int32_t* p4 = reinterpret_cast<const int32_t*>(wblock + kWireHdr);
            const int32_t pk0 = p4[sub], pk1 = p4[32 + sub];
            float4_ev o0{}, o1{};
            if constexpr (ACC) {
                o0 = *reinterpret_cast<const float4_ev*>(obase + sub * 4);
                o1 = *reinterpret_cast<const float4_ev*>(obase + 128 + sub * 4);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                o0[j] = DequantElem<T, ACC>(QUnpack(pk0, j), scale, o0[j]);
                o1[j] = DequantElem<T, ACC>(QUnpack(pk1, j), scale, o1[j]);
            }
            StoreVec<NT_ST>(o0, obase + sub * 4);
            StoreVec<NT_ST>(o1, obase + 128 + sub * 4);
        } else {
            const uint2_ev packed =
                *reinterpret_cast<const uint2_ev*>(wblock + kWireHdr + sub * 8);
            ushort8_t v{};
            if constexpr (ACC) v = *reinterpret_cast<const ushort8_t*>(obase + sub * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                v[j] = DequantElem<T, ACC>(QUnpack(packed[j >> 2], j & 3), scale, v[j]);
            StoreVec<NT_ST>(v, obase + sub * 8);
        }
    });
}

template <typename T>
void DequantizeSegmentsTyped(const uint8_t* wire, size_t nseg, void* out, size_t count,
                             size_t block_elems, bool accumulate, hipStream_t stream) {
    const size_t nblocks = NumBlocks(count, block_elems);
    const size_t total = nseg * nblocks;
    T* o = static_cast<T*>(out);
    const bool x2 = block_elems == kFastBlock && count % kFastBlock == 0 &&
                    (reinterpret_cast<uintptr_t>(out) & 15) == 0 &&
                    (reinterpret_cast<uintptr_t>(wire) & 7) == 0;
    // Assign mode on the fast path could go to LaunchDequantize's flat kernels
    // (same bits). Measured at 64 Mi elements, 2 to 8 segments: this kernel
    // 68 us against 87 us for f32, 49 us against 49 us for bf16
    // (docs/BENCHMARKS.md), so it keeps both modes.
    DispatchBool(accumulate, [&](auto acc) {
        constexpr bool ACC = decltype(acc)::value;
        if (x2) {
            // nontemporal stores under LaunchQuantSumDequant's rule
            DispatchBool(nseg * count * sizeof(T) >= kSumDequantNtBytes, [&](auto nt) {
                DequantizeSegmentsX2Kernel<T, ACC, decltype(nt)::value>
                    <<<PairGrid(total), dim3(kBlock), 0, stream>>>(wire, o, total);
            });
        } else {
            MLSL_CHECK(total <= 0xffffffffull, "segmented dequantize: too many wire blocks");
            DequantizeSegmentsKernel<T, ACC><<<WaveGrid(total), dim3(kBlock), 0, stream>>>(
                wire, o, count, block_elems, static_cast<uint32_t>(nblocks),
                MakeFastDiv(static_cast<uint32_t>(nblocks)), static_cast<uint32_t>(total));
        }
    });
}

}  // namespace

void LaunchDequantizeSegments(const void* wire, size_t nseg, void* out, size_t count,
                              size_t block_elems, DataType dt, bool accumulate,
                              hipStream_t stream) {
    CheckQuantBlock(block_elems, "LaunchDequantizeSegments");
    if (dt != DataType::F32 && dt != DataType::BF16)
        MLSL_THROW("segmented dequantize supports f32/bf16 only");
    MLSL_CHECK(nseg >= 1, "segmented dequantize takes at least one segment");
    if (count == 0) return;
    const uint8_t* w = static_cast<const uint8_t*>(wire);
    if (dt == DataType::F32)
        DequantizeSegmentsTyped<float>(w, nseg, out, count, block_elems, accumulate, stream);
    else
        DequantizeSegmentsTyped<unsigned short>(w, nseg, out, count, block_elems, accumulate,
                                                stream);
    HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// Quantize from, and dequantize into, a list of tensors: the prologue and the
// finish of the allreduce over a list (DDP gradient buckets). The
// concatenation V of the nseg tensors is never materialised: the wire's block
// grid runs over V's element index, tensor j holds V[offs[j], offs[j + 1]),
// and both tables (nseg + 1 prefix offsets, nseg pointers) are read from
// device memory. A wave finds the tensor of its block's first element once,
// by a wave-uniform bisection of the offsets. A block that lies inside one
// tensor, at a 16-byte aligned address, then runs the flat kernels' 4-wide
// loop on that tensor (a whole 256-block of the gather: four elements per
// lane, read once and kept in registers); any other block goes element by
// element, every lane walking forward through the table from the block's
// first tensor. The wave keeps its tensor from one block to its next.
//
// Traffic per element is the flat kernels': sizeof(T) in (twice that with a
// residual, which is also written) and 1 wire byte out, or 1 wire byte in and
// sizeof(T) out; plus one bisection of 8-byte offsets per block.

namespace {

struct SegTable {
    const uint64_t* offs;   // nseg + 1 prefix offsets in elements; offs[0] == 0
    uint32_t nseg;
};

// Largest j with offs[j] <= idx, for idx < offs[nseg], given offs[lo] <= idx.
__device__ __forceinline__ uint32_t SegOf(const SegTable& t, uint64_t idx, uint32_t lo) {
    uint32_t hi = t.nseg;
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (t.offs[mid] <= idx) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The tensor of a wave's current block, kept across its grid-stride trips: a
// wave's blocks ascend, so a block inside the tensor of the last one costs no
// table read, and any other is found by a bisection that starts there.
template <typename T>
struct SegCursor {
    uint32_t seg = 0;
    uint64_t lo = 0, hi = 0;   // the tensor holds V[lo, hi); hi == 0: none yet
    T* ptr = nullptr;
    template <typename P>
    __device__ __forceinline__ void Seek(const SegTable& t, P ptrs, uint64_t base) {
        if (base < hi) return;
        seg = SegOf(t, base, seg);
        lo = t.offs[seg];
        hi = t.offs[seg + 1];
        ptr = ptrs[seg];
    }
};

// f(i, p) for the elements i = lane, lane + 64, ... < n of the block that
// starts at V[base], p pointing at element base + i in its tensor. `c` is at
// the tensor of V[base]; the lane's own cursor only ever moves forward.
template <typename T, typename P, typename F>
__device__ __forceinline__ void ForEachSegElem(const SegTable& t, P ptrs,
                                               const SegCursor<T>& c, uint64_t base, size_t n,
                                               int lane, F f) {
    uint32_t s = c.seg;
    uint64_t lo = c.lo, hi = c.hi;
    T* p = c.ptr;
    for (size_t i = lane; i < n; i += 64) {
        const uint64_t e = base + i;
        if (e >= hi) {
            // the table's last entry bounds the walk whatever `count` says
            while (e >= hi && s + 1 < t.nseg) hi = t.offs[++s + 1];
            lo = t.offs[s];
            p = ptrs[s];
        }
        f(i, p + (e - lo));
    }
}

// One wire block of a list: the n >= 1 elements that start at V[base], `cur`
// at the tensor of V[base], the block's residual at eb (null without USE_ERR).
// Writes the header, the payload (zero from n up to block_elems) and the
// residual of the n elements. QuantizeKernel's arithmetic per element, on one
// of three paths, chosen per block: 256 elements inside one tensor with the
// tensor address and eb both 16-byte aligned stay in registers, four
// consecutive elements per lane read once; a block inside one tensor at an
// aligned address takes the 4-wide loop; any other walks the table.
template <typename T, bool USE_ERR, typename P>
__device__ __forceinline__ void QuantizeSegBlock(const SegTable& tab, P ptrs,
                                                 const SegCursor<const T>& cur, size_t base,
                                                 size_t n, size_t block_elems, T* eb,
                                                 uint8_t* wblock, int lane) {
    using V4 = std::conditional_t<sizeof(T) == 4, float4_ev, ushort4_t>;
    int8_t* payload = reinterpret_cast<int8_t*>(wblock + kWireHdr);
    const T* in = cur.ptr + (base - cur.lo);   // V[base], if the block is whole
    const bool whole = base + n <= cur.hi;
    const bool aligned = (reinterpret_cast<uintptr_t>(in) & 15) == 0;
    const bool regs = block_elems == kFastBlock && n == kFastBlock &&
                      (reinterpret_cast<uintptr_t>(eb) & 15) == 0;

    if (whole && aligned && regs) {
        const V4 a = *reinterpret_cast<const V4*>(in + lane * 4);
        V4 e{};
        if (USE_ERR) e = *reinterpret_cast<const V4*>(eb + lane * 4);
        float v[4];
        float m = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = Decode<T>(a[k]);
            if (USE_ERR) v[k] += Decode<T>(e[k]);
            m = fmaxf(m, fabsf(v[k]));
        }
        const float scale = QScale(WaveMax(m));
        if (lane == 0) WriteWireHeader(wblock, scale);
        const float inv = 1.f / scale;
        uint32_t packed = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float q = QRound(v[k], inv);
            packed |= QPack(q, k);
            if (USE_ERR) e[k] = Encode<T>(v[k] - q * scale);
        }
        QStore<4>(payload, lane * 4, packed);
        if (USE_ERR) StoreVec<false>(e, eb + lane * 4);
    } else if (whole && aligned) {
        auto value = [&](size_t i) {
            float v = Decode(in[i]);
            if (USE_ERR) v += Decode(eb[i]);
            return v;
        };
        float m = 0.f;
        ForEachBlockElem(n, true, lane, [&](size_t i, auto w) {
#pragma unroll
            for (int k = 0; k < decltype(w)::value; ++k)
                m = fmaxf(m, fabsf(value(i + k)));
        });
        const float scale = QScale(WaveMax(m));
        if (lane == 0) WriteWireHeader(wblock, scale);
        const float inv = 1.f / scale;
        ForEachBlockElem(n, true, lane, [&](size_t i, auto w) {
            constexpr int W = decltype(w)::value;
            uint32_t packed = 0;
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const float v = value(i + k);
                const float q = QRound(v, inv);
                packed |= QPack(q, k);
                if (USE_ERR) eb[i + k] = Encode<T>(v - q * scale);
            }
            QStore<W>(payload, i, packed);
        });
    } else {
        auto value = [&](size_t i, const T* p) {
            float v = Decode(*p);
            if (USE_ERR) v += Decode(eb[i]);
            return v;
        };
        float m = 0.f;
        ForEachSegElem<const T>(tab, ptrs, cur, base, n, lane,
                                [&](size_t i, const T* p) {
                                    m = fmaxf(m, fabsf(value(i, p)));
                                });
        const float scale = QScale(WaveMax(m));
        if (lane == 0) WriteWireHeader(wblock, scale);
        const float inv = 1.f / scale;
        ForEachSegElem<const T>(tab, ptrs, cur, base, n, lane,
                                [&](size_t i, const T* p) {
                                    const float v = value(i, p);
                                    const float q = QRound(v, inv);
                                    payload[i] = static_cast<int8_t>(q);
                                    if (USE_ERR) eb[i] = Encode<T>(v - q * scale);
                                });
    }
    // whatever the block holds past its n elements
    for (size_t i = n + lane; i < block_elems; i += 64) payload[i] = 0;
}

template <typename T, bool USE_ERR>
__global__ void QuantizeGatherKernel(const T* const* __restrict__ ptrs, SegTable tab,
                                     T* __restrict__ err, uint8_t* __restrict__ wire,
                                     size_t count, size_t block_elems) {
    SegCursor<const T> cur;
    ForEachWaveBlock((count + block_elems - 1) / block_elems, [&](size_t vblk, int lane) {
        // uniform across the wave: the bisection and the table reads stay in
        // scalar registers
        const size_t blk = (static_cast<size_t>(__builtin_amdgcn_readfirstlane(
                                static_cast<uint32_t>(vblk >> 32))) << 32) |
                           __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(vblk));
        const size_t base = blk * block_elems;
        cur.Seek(tab, ptrs, base);
        QuantizeSegBlock<T, USE_ERR>(tab, ptrs, cur, base, min(block_elems, count - base),
                                     block_elems, USE_ERR ? err + base : nullptr,
                                     wire + blk * (block_elems + kWireHdr), lane);
    });
}

// The prologue of the reduce-scatter over a list: V' is the concatenation V
// (total elements) followed by zeros up to nshards * shard, and shard j, V'[j *
// shard, (j + 1) * shard), is quantized on a block grid of its own into wire +
// j * wire_stride, with the residual flat in V' order. One launch covers all
// shards: wire block `blk` of the launch is block blk % bps of shard blk / bps,
// so block bases still ascend with blk and the cursor only moves forward.
// What differs from QuantizeGatherKernel: a block's base in V' is j * shard +
// b * block_elems, no multiple of anything, so the alignment of the tensor
// address AND of err + base is looked at per block; and an element at or past
// `total` is the value 0 and is never looked up: only the block's `real`
// elements go through the table or touch the residual (a padding element's
// residual is +0 and stays so), and a block at or past `total` is all zero.
template <typename T, bool USE_ERR>
__global__ void QuantizeGatherShardsKernel(const T* const* __restrict__ ptrs, SegTable tab,
                                           T* __restrict__ err, uint8_t* __restrict__ wire,
                                           size_t total, uint32_t nshards, size_t shard,
                                           size_t wire_stride, size_t block_elems) {
    SegCursor<const T> cur;
    const uint32_t bps = static_cast<uint32_t>((shard + block_elems - 1) / block_elems);
    ForEachWaveBlock(static_cast<size_t>(nshards) * bps, [&](size_t vblk, int lane) {
        // uniform across the wave (the launcher keeps the block count in 32 bits)
        const uint32_t blk = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(vblk));
        const uint32_t j = blk / bps, b = blk - j * bps;
        const size_t in_shard = static_cast<size_t>(b) * block_elems;
        const size_t base = static_cast<size_t>(j) * shard + in_shard;
        const size_t n = min(block_elems, shard - in_shard);
        uint8_t* wblock = wire + j * wire_stride + static_cast<size_t>(b) * (block_elems + kWireHdr);
        int8_t* payload = reinterpret_cast<int8_t*>(wblock + kWireHdr);
        if (base >= total) {
            // padding only: nothing is read. An early return on purpose: with
            // the count of real elements written as one expression, base <
            // total ? min(n, total - base) : 0, blocks past `total` were seen
            // to go through the table on the device.
            if (lane == 0) WriteWireHeader(wblock, QScale(0.f));
            for (size_t i = lane * 4; i < block_elems; i += 256) QStore<4>(payload, i, 0);
            return;
        }
        // the block's elements that exist: at least one from here on
        const size_t real = min(n, total - base);
        cur.Seek(tab, ptrs, base);
        QuantizeSegBlock<T, USE_ERR>(tab, ptrs, cur, base, real, block_elems,
                                     USE_ERR ? err + base : nullptr, wblock, lane);
    });
}

// ROUND_FIRST (bf16 only; f32 would not change): q * scale is rounded into T
// before it is scaled, which is what LaunchDequantize followed by a
// multiplication of the stored elements gives.
template <typename T, bool ROUND_FIRST>
__global__ void DequantizeScatterKernel(const uint8_t* __restrict__ wire, T* const* ptrs,
                                        SegTable tab, size_t count, size_t block_elems,
                                        float post_scale) {
    SegCursor<T> cur;
    ForEachWaveBlock((count + block_elems - 1) / block_elems, [&](size_t vblk, int lane) {
        const size_t blk = (static_cast<size_t>(__builtin_amdgcn_readfirstlane(
                                static_cast<uint32_t>(vblk >> 32))) << 32) |
                           __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(vblk));
        const size_t base = blk * block_elems;
        const size_t n = min(block_elems, count - base);
        const uint8_t* wblock = wire + blk * (block_elems + kWireHdr);
        const float scale = WireScale(wblock);
        const int8_t* payload = reinterpret_cast<const int8_t*>(wblock + kWireHdr);
        cur.Seek(tab, ptrs, base);
        T* out = cur.ptr + (base - cur.lo);
        const bool whole = base + n <= cur.hi;
        // two roundings to float, then one into T: never (scale * post_scale)
        auto elem = [&](int q) {
            float dq = q * scale;
            if constexpr (ROUND_FIRST) dq = Decode<T>(Encode<T>(dq));
            return Encode<T>(dq * post_scale);
        };

        if (whole && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {
            ForEachBlockElem(n, true, lane, [&](size_t i, auto w) {
                constexpr int W = decltype(w)::value;
                const int32_t packed = QLoad<W>(payload, i);
                if constexpr (W == 4) {
                    using V = std::conditional_t<sizeof(T) == 4, float4_ev, ushort4_t>;
                    V v;
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = elem(QUnpack(packed, j));
                    StoreVec<false>(v, out + i);
                } else {
                    out[i] = elem(QUnpack(packed, 0));
                }
            });
        } else {
            ForEachSegElem<T>(tab, ptrs, cur, base, n, lane,
                              [&](size_t i, T* p) { *p = elem(payload[i]); });
        }
    });
}

void CheckSegArgs(const void* ptrs, const void* offs, size_t nseg, size_t count, DataType dt,
                  const char* where) {
    if (dt != DataType::F32 && dt != DataType::BF16)
        MLSL_THROW(std::string(where) + " supports f32/bf16 only");
    MLSL_CHECK(nseg >= 1 && nseg <= 0xffffffffull && count >= nseg,
               std::string(where) + " takes at least one segment of at least one element");
    MLSL_CHECK(ptrs != nullptr && offs != nullptr,
               std::string(where) + ": null segment table");
}

}  // namespace

void LaunchQuantizeGather(const void* const* seg_ptrs, const uint64_t* seg_offs, size_t nseg,
                          void* err, void* wire, size_t count, size_t block_elems,
                          DataType dt, bool use_err, hipStream_t stream) {
    CheckQuantBlock(block_elems, "LaunchQuantizeGather");
    CheckSegArgs(seg_ptrs, seg_offs, nseg, count, dt, "quantize-gather");
    const SegTable tab{seg_offs, static_cast<uint32_t>(nseg)};
    const dim3 grid = WaveGrid(NumBlocks(count, block_elems));
    uint8_t* w = static_cast<uint8_t*>(wire);
    DispatchBool(use_err, [&](auto ue) {
        constexpr bool UE = decltype(ue)::value;
        if (dt == DataType::F32)
            QuantizeGatherKernel<float, UE><<<grid, dim3(kBlock), 0, stream>>>(
                reinterpret_cast<const float* const*>(seg_ptrs), tab,
                static_cast<float*>(err), w, count, block_elems);
        else
            QuantizeGatherKernel<unsigned short, UE><<<grid, dim3(kBlock), 0, stream>>>(
                reinterpret_cast<const unsigned short* const*>(seg_ptrs), tab,
                static_cast<unsigned short*>(err), w, count, block_elems);
    });
    HIP_CHECK(hipGetLastError());
}

void LaunchQuantizeGatherShards(const void* const* seg_ptrs, const uint64_t* seg_offs,
                                size_t nseg, void* err, void* wire, size_t total,
                                size_t nshards, size_t shard, size_t wire_stride,
                                size_t block_elems, DataType dt, bool use_err,
                                hipStream_t stream) {
    CheckQuantBlock(block_elems, "LaunchQuantizeGatherShards");
    CheckSegArgs(seg_ptrs, seg_offs, nseg, total, dt, "quantize-gather-shards");
    MLSL_CHECK(nshards >= 1 && shard >= (total + nshards - 1) / nshards,
               "quantize-gather-shards: shard * nshards < total (the shards do not hold "
               "the tensors)");
    const size_t bps = NumBlocks(shard, block_elems);
    MLSL_CHECK(bps * nshards <= 0xffffffffull,
               "quantize-gather-shards: more than 2^32 wire blocks");
    // a wire block needs its header's and its payload words' alignment only
    MLSL_CHECK(wire_stride % 4 == 0 && wire_stride >= bps * (block_elems + kWireHdr),
               "quantize-gather-shards: wire_stride is smaller than one shard's wire or "
               "no multiple of 4");
    MLSL_CHECK(!use_err || err != nullptr, "quantize-gather-shards: use_err without err");
    const SegTable tab{seg_offs, static_cast<uint32_t>(nseg)};
    const dim3 grid = WaveGrid(bps * nshards);
    uint8_t* w = static_cast<uint8_t*>(wire);
    DispatchBool(use_err, [&](auto ue) {
        constexpr bool UE = decltype(ue)::value;
        if (dt == DataType::F32)
            QuantizeGatherShardsKernel<float, UE><<<grid, dim3(kBlock), 0, stream>>>(
                reinterpret_cast<const float* const*>(seg_ptrs), tab,
                static_cast<float*>(err), w, total, static_cast<uint32_t>(nshards), shard,
                wire_stride, block_elems);
        else
            QuantizeGatherShardsKernel<unsigned short, UE><<<grid, dim3(kBlock), 0, stream>>>(
                reinterpret_cast<const unsigned short* const*>(seg_ptrs), tab,
                static_cast<unsigned short*>(err), w, total, static_cast<uint32_t>(nshards),
                shard, wire_stride, block_elems);
    });
    HIP_CHECK(hipGetLastError());
}

void LaunchDequantizeScatter(const void* wire, void* const* seg_ptrs,
                             const uint64_t* seg_offs, size_t nseg, size_t count,
                             size_t block_elems, DataType dt, float post_scale,
                             bool round_first, hipStream_t stream) {
    CheckQuantBlock(block_elems, "LaunchDequantizeScatter");
    CheckSegArgs(seg_ptrs, seg_offs, nseg, count, dt, "dequantize-scatter");
    const SegTable tab{seg_offs, static_cast<uint32_t>(nseg)};
    const dim3 grid = WaveGrid(NumBlocks(count, block_elems));
    const uint8_t* w = static_cast<const uint8_t*>(wire);
    if (dt == DataType::F32) {
        // q * scale already is an f32: rounding it first changes nothing
        DequantizeScatterKernel<float, false><<<grid, dim3(kBlock), 0, stream>>>(
            w, reinterpret_cast<float* const*>(seg_ptrs), tab, count, block_elems, post_scale);
    } else {
        DispatchBool(round_first, [&](auto rf) {
            DequantizeScatterKernel<unsigned short, decltype(rf)::value>
                <<<grid, dim3(kBlock), 0, stream>>>(
                    w, reinterpret_cast<unsigned short* const*>(seg_ptrs), tab, count,
                    block_elems, post_scale);
        });
    }
    HIP_CHECK(hipGetLastError());
}

// --- IPC p2p transport (comm/p2p_transport.cpp) ---
// Mailboxes are monotonically increasing u64 sequence counters in the
// receiver's HBM window; the writer is a remote process on the same or a
// peer GPU, so both sides use system-scope atomics. Every wait has TWO
// escape hatches so a lost peer can never wedge the GPU: a host-written
// abort word (pinned) and a wall-clock bound (s_memrealtime, 100 MHz).
// On escape it writes 1 to `status` (pinned) and returns — the host
// request machinery sees it and fails the request loudly.

namespace {

struct PollArgs {
    const unsigned long long* mbox;  // null = no wait
    unsigned long long target;
    const unsigned int* abort_word;
    unsigned int* status;
    unsigned long long max_ticks;
};

PollArgs ToPollArgs(const XferPoll* p) {
    PollArgs pa{};
    if (p) {
        pa.mbox = static_cast<const unsigned long long*>(p->mbox);
        pa.target = p->target;
        pa.abort_word = static_cast<const unsigned int*>(p->abort_word);
        pa.status = static_cast<unsigned int*>(p->status);
        pa.max_ticks = p->max_ticks;
    }
    return pa;
}

inline unsigned long long* U64(void* p) { return static_cast<unsigned long long*>(p); }

// One lane spins until *mbox >= target with RELAXED loads (consumer recipe,
// MI355X_MICROARCH.md: polling with acquire loads is correct but 2-3x
// slower per hop and cuts chip bandwidth with many pollers); the caller
// acquires once afterwards. Returns false, with 1 stored to *ab.status, on
// abort or when the wall clock passes t0 + ab.max_ticks.
__device__ __forceinline__ bool SpinGeq(const unsigned long long* mbox,
                                        unsigned long long target,
                                        const PollArgs& ab, unsigned long long t0) {
    while (__hip_atomic_load(mbox, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) <
           target) {
        if (__hip_atomic_load(ab.abort_word, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_SYSTEM) != 0 ||
            wall_clock64() - t0 > ab.max_ticks) {
            __hip_atomic_store(ab.status, 1u, __ATOMIC_RELEASE,
                               __HIP_MEMORY_SCOPE_SYSTEM);
            return false;
        }
        __builtin_amdgcn_s_sleep(64);
    }
    return true;
}

// Stream-blocking wait: one lane, then the acquire (consumers in the NEXT
// kernel get their visibility from the dispatch boundary; this orders
// same-stream work).
__global__ void WaitFlagKernel(PollArgs pa) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (SpinGeq(pa.mbox, pa.target, pa, wall_clock64()))
        (void)__hip_atomic_load(pa.mbox, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ void SetFlagKernel(unsigned long long* __restrict__ mbox,
                              unsigned long long val) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(mbox, val, __ATOMIC_RELEASE,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// Poll prologue of the payload kernels: thread 0 of every workgroup waits
// for mbox >= target, then the workgroup proceeds — one kernel instead of
// wait-kernel + work-kernel. False means aborted: the workgroup returns.
__device__ __forceinline__ bool PollGeq(const unsigned long long* mbox,
                                        unsigned long long target,
                                        const PollArgs& ab) {
    __shared__ int ok;
    if (threadIdx.x == 0) {
        ok = 1;
        if (SpinGeq(mbox, target, ab, wall_clock64()))
            (void)__hip_atomic_load(mbox, __ATOMIC_ACQUIRE,
                                    __HIP_MEMORY_SCOPE_SYSTEM);
        else
            ok = 0;
    }
    __syncthreads();
    return ok != 0;
}

// Byte copy of a payload into a hand-off slot: 16-B vectors + byte tail,
// bytewise when either side is unaligned. PLAIN stores (MI355X_MICROARCH.md:
// "never nt on hand-off stores" — nt bypasses the cache hierarchy without
// probing, so a consumer-side cached line can shadow it); the NT load of
// the local source is safe and streams past L2.
__device__ __forceinline__ void SlotCopy(uint8_t* __restrict__ dst,
                                         const uint8_t* __restrict__ src,
                                         size_t bytes, size_t tid, size_t stride) {
    const bool al = ((reinterpret_cast<uintptr_t>(dst) |
                      reinterpret_cast<uintptr_t>(src)) & 15) == 0;
    if (al) {
        const size_t n16 = bytes / 16;
        const uint4_ev* s = reinterpret_cast<const uint4_ev*>(src);
        uint4_ev* d = reinterpret_cast<uint4_ev*>(dst);
        for (size_t i = tid; i < n16; i += stride)
            d[i] = __builtin_nontemporal_load(s + i);
        for (size_t j = n16 * 16 + tid; j < bytes; j += stride) dst[j] = src[j];
    } else {
        for (size_t j = tid; j < bytes; j += stride) dst[j] = src[j];
    }
}

// byte copy with optional poll prologue. The publish (in_flag/ack) after
// the wide Xfer kernels is a separate 1-wg SetFlag kernel so stream order
// provides the grid-completion barrier without cooperative launch.
__global__ void XferCopyKernel(uint8_t* __restrict__ dst,
                               const uint8_t* __restrict__ src, size_t bytes,
                               PollArgs pa) {
    if (pa.mbox && !PollGeq(pa.mbox, pa.target, pa)) return;
    SlotCopy(dst, src, bytes, blockIdx.x * blockDim.x + threadIdx.x,
             gridDim.x * blockDim.x);
}

// dst (op)= slot  |  dst = slot (op) other   — f32, vec4 when aligned
template <ReduceOp OP, bool OUT>
__global__ void XferReduceF32Kernel(float* __restrict__ dst,
                                    const float* __restrict__ slot,
                                    const float* __restrict__ other, size_t n,
                                    PollArgs pa) {
    if (pa.mbox && !PollGeq(pa.mbox, pa.target, pa)) return;
    const size_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = gridDim.x * blockDim.x;
    const bool al = ((reinterpret_cast<uintptr_t>(dst) |
                      reinterpret_cast<uintptr_t>(slot) |
                      reinterpret_cast<uintptr_t>(other)) & 15) == 0;
    if (al) {
        const size_t n4 = n / 4;
        const float4_ev* s4 = reinterpret_cast<const float4_ev*>(slot);
        const float4_ev* o4 = reinterpret_cast<const float4_ev*>(other);
        float4_ev* d4 = reinterpret_cast<float4_ev*>(dst);
        // plain accesses throughout (hand-off rule; the slot was written
        // by another process, the output feeds later sends)
        for (size_t i = tid; i < n4; i += stride)
            d4[i] = CombineVec<float, OP, 4>(OUT ? o4[i] : d4[i], s4[i]);
        for (size_t j = n4 * 4 + tid; j < n; j += stride)
            dst[j] = Apply<float, OP>(OUT ? other[j] : dst[j], slot[j]);
    } else {
        for (size_t j = tid; j < n; j += stride)
            dst[j] = Apply<float, OP>(OUT ? other[j] : dst[j], slot[j]);
    }
}

template <ReduceOp OP, bool OUT>
__global__ void XferReduceBf16Kernel(unsigned short* __restrict__ dst,
                                     const unsigned short* __restrict__ slot,
                                     const unsigned short* __restrict__ other,
                                     size_t n, PollArgs pa) {
    if (pa.mbox && !PollGeq(pa.mbox, pa.target, pa)) return;
    const size_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = gridDim.x * blockDim.x;
    for (size_t j = tid; j < n; j += stride)
        dst[j] = Combine<unsigned short, OP>(OUT ? other[j] : dst[j], slot[j]);
}

}  // namespace

void LaunchXferCopy(void* dst, const void* src, size_t bytes,
                    const XferPoll* poll, hipStream_t stream) {
    XferCopyKernel<<<dim3(GridFor(bytes / 16 + 1)), dim3(kBlock), 0, stream>>>(
        static_cast<uint8_t*>(dst), static_cast<const uint8_t*>(src), bytes,
        ToPollArgs(poll));
    HIP_CHECK(hipGetLastError());
}

bool LaunchXferReduce(void* dst, const void* slot, const void* other, size_t n,
                      DataType dt, ReduceOp op, const XferPoll* poll,
                      hipStream_t stream) {
    if (dt != DataType::F32 && dt != DataType::BF16)
        return false;  // caller falls back to wait + LaunchReduce
    const PollArgs pa = ToPollArgs(poll);
    const dim3 grid(GridFor(n / 4 + 1));
    DispatchOp(op, [&](auto o) {
        DispatchBool(other != nullptr, [&](auto out) {
            constexpr ReduceOp OP = decltype(o)::value;
            constexpr bool OUT = decltype(out)::value;
            if (dt == DataType::F32)
                XferReduceF32Kernel<OP, OUT><<<grid, dim3(kBlock), 0, stream>>>(
                    static_cast<float*>(dst), static_cast<const float*>(slot),
                    static_cast<const float*>(other), n, pa);
            else
                XferReduceBf16Kernel<OP, OUT><<<grid, dim3(kBlock), 0, stream>>>(
                    static_cast<unsigned short*>(dst),
                    static_cast<const unsigned short*>(slot),
                    static_cast<const unsigned short*>(other), n, pa);
        });
    });
    HIP_CHECK(hipGetLastError());
    return true;
}

// --- fully-fused small-message transport kernels ---
// One kernel per side per sub-message: poll prologue + payload + grid-
// completion counter + flag publish. The grid is FIXED at kXferFusedGrid
// workgroups so a spinning kernel can never starve the peer's consumer of
// CUs (the full-device fused-poll variant deadlocked two ranks; 2-4 ranks
// x a few 32-wg spinners always co-schedule on 256 CUs). Completion is
// detected with a monotonic per-edge counter: every workgroup does a
// system-scope acq_rel fetch-add; the one that observes target-1 publishes
// the flag(s) with system release stores — which also orders every other
// workgroup's payload writes (their adds released them).

namespace {

__device__ __forceinline__ void FusedFinish(unsigned long long* ctr,
                                            unsigned long long target,
                                            unsigned long long* const* mbox,
                                            const unsigned long long* val,
                                            int nflags) {
    __syncthreads();
    if (threadIdx.x == 0) {
        // ROCm 7.2 / gfx950 compiler hazard (MI355X_MICROARCH.md): when the
        // publishing wave's vmcnt scoreboard looks provably empty, the
        // compiler drops the s_waitcnt after the release's buffer_wbl2 and
        // the flag can overtake the payload write-back (~1e-4 stale under
        // load — observed as a zero arrival row in the ring RS). Inline asm
        // is invisible to that pass: force the wait before the release-add
        // and again before the publish store.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned long long prev = __hip_atomic_fetch_add(
            ctr, 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_SYSTEM);
        if (prev == target - 1) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            for (int p = 0; p < nflags; ++p)
                __hip_atomic_store(mbox[p], val[p], __ATOMIC_RELEASE,
                                   __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

__device__ __forceinline__ void FusedFinish(unsigned long long* ctr,
                                            unsigned long long target,
                                            unsigned long long* mbox,
                                            unsigned long long val) {
    FusedFinish(ctr, target, &mbox, &val, 1);
}

// sender: [backpressure poll] + byte copy into the peer slot + publish
__global__ void XferSendFusedKernel(uint8_t* __restrict__ slot,
                                    const uint8_t* __restrict__ src,
                                    size_t bytes, PollArgs bp,
                                    unsigned long long* ctr,
                                    unsigned long long ctr_target,
                                    unsigned long long* in_mbox,
                                    unsigned long long seq) {
    if (bp.mbox && !PollGeq(bp.mbox, bp.target, bp)) return;
    SlotCopy(slot, src, bytes, blockIdx.x * blockDim.x + threadIdx.x,
             gridDim.x * blockDim.x);
    FusedFinish(ctr, ctr_target, in_mbox, seq);
}

// receiver: arrival poll + consume (copy / reduce / reduce-out) + ack
template <typename T, ReduceOp OP, FusedConsume MODE>
__global__ void XferRecvFusedKernel(T* __restrict__ dst,
                                    const T* __restrict__ slot,
                                    const T* __restrict__ other, size_t n,
                                    PollArgs wp, unsigned long long* ctr,
                                    unsigned long long ctr_target,
                                    unsigned long long* ack_mbox,
                                    unsigned long long seq) {
    if (!PollGeq(wp.mbox, wp.target, wp)) return;
    const size_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = gridDim.x * blockDim.x;
    for (size_t j = tid; j < n; j += stride) {
        if constexpr (MODE == FusedConsume::COPY)
            dst[j] = slot[j];
        else
            dst[j] = Combine<T, OP>(
                MODE == FusedConsume::REDUCE ? dst[j] : other[j], slot[j]);
    }
    FusedFinish(ctr, ctr_target, ack_mbox, seq);
}

// fused arrival-wait + compressed-domain accumulate (quantized ring)
__global__ void XferRecvQuantAccumKernel(uint8_t* __restrict__ acc,
                                         const uint8_t* __restrict__ slot,
                                         size_t count, size_t block_elems,
                                         PollArgs wp, unsigned long long* ctr,
                                         unsigned long long ctr_target,
                                         unsigned long long* ack_mbox,
                                         unsigned long long seq) {
    if (!PollGeq(wp.mbox, wp.target, wp)) return;
    QuantAccumBody(acc, slot, count, block_elems);
    FusedFinish(ctr, ctr_target, ack_mbox, seq);
}

}  // namespace

void LaunchXferSendFused(void* slot, const void* src, size_t bytes,
                         const XferPoll* bp, void* ctr, uint64_t ctr_target,
                         void* in_mbox, uint64_t seq, hipStream_t stream) {
    XferSendFusedKernel<<<dim3(kXferFusedGrid), dim3(kBlock), 0, stream>>>(
        static_cast<uint8_t*>(slot), static_cast<const uint8_t*>(src), bytes,
        ToPollArgs(bp), U64(ctr), ctr_target, U64(in_mbox), seq);
    HIP_CHECK(hipGetLastError());
}

bool LaunchXferRecvFused(void* dst, const void* slot, const void* other,
                         size_t n, DataType dt, ReduceOp op, FusedConsume mode,
                         const XferPoll* wp, void* ctr, uint64_t ctr_target,
                         void* ack_mbox, uint64_t seq, hipStream_t stream) {
    const PollArgs pa = ToPollArgs(wp);
    auto launch = [&](auto* typed_dst, auto o, auto m) {
        using T = std::remove_pointer_t<decltype(typed_dst)>;
        XferRecvFusedKernel<T, decltype(o)::value, decltype(m)::value>
            <<<dim3(kXferFusedGrid), dim3(kBlock), 0, stream>>>(
                typed_dst, static_cast<const T*>(slot), static_cast<const T*>(other),
                n, pa, U64(ctr), ctr_target, U64(ack_mbox), seq);
    };
    using Sum = std::integral_constant<ReduceOp, ReduceOp::SUM>;
    using Copy = std::integral_constant<FusedConsume, FusedConsume::COPY>;
    using Reduce = std::integral_constant<FusedConsume, FusedConsume::REDUCE>;
    using ReduceOut = std::integral_constant<FusedConsume, FusedConsume::REDUCE_OUT>;
    if (mode == FusedConsume::COPY) {
        launch(static_cast<uint8_t*>(dst), Sum{}, Copy{});  // byte copy, dtype-agnostic
    } else if (dt == DataType::F32 || dt == DataType::BF16) {
        DispatchOp(op, [&](auto o) {
            DispatchBool(mode == FusedConsume::REDUCE_OUT, [&](auto out) {
                using M = std::conditional_t<decltype(out)::value, ReduceOut, Reduce>;
                if (dt == DataType::F32) launch(static_cast<float*>(dst), o, M{});
                else launch(static_cast<unsigned short*>(dst), o, M{});
            });
        });
    } else {
        return false;
    }
    HIP_CHECK(hipGetLastError());
    return true;
}

void LaunchXferRecvQuantAccum(void* acc, const void* slot, size_t count,
                              size_t block_elems, const XferPoll* wp,
                              void* ctr, uint64_t ctr_target, void* ack_mbox,
                              uint64_t seq, hipStream_t stream) {
    XferRecvQuantAccumKernel<<<dim3(kXferFusedGrid), dim3(kBlock), 0, stream>>>(
        static_cast<uint8_t*>(acc), static_cast<const uint8_t*>(slot), count,
        block_elems, ToPollArgs(wp), U64(ctr), ctr_target, U64(ack_mbox), seq);
    HIP_CHECK(hipGetLastError());
}

// --- one-shot (direct) allreduce fan kernels ---
// Fan-out: ONE kernel pushes the payload to every peer's slot (4 wgs per
// peer, per-peer backpressure poll + publish). Fan-in: ONE kernel waits
// for all arrivals, then reduces them into dst in a single pass (P slot
// reads + 1 dst read + 1 dst write per element) and publishes every ack.
// Small-message allreduce becomes 2 transport kernels regardless of N.

namespace {

struct FanKernArgs {
    void* slot[8];
    unsigned long long* flag[8];
    unsigned long long flag_val[8];
    const unsigned long long* wait_mbox[8];
    unsigned long long wait_target[8];
    unsigned long long* ctr[8];
    unsigned long long ctr_target[8];
    int npeers;
};

__global__ void FanOutSendKernel(const uint8_t* __restrict__ src, size_t bytes,
                                 FanKernArgs fa, PollArgs ab, int wgs_per_peer) {
    const int p = blockIdx.x / wgs_per_peer;
    if (p >= fa.npeers) return;
    if (fa.wait_mbox[p] && !PollGeq(fa.wait_mbox[p], fa.wait_target[p], ab))
        return;
    SlotCopy(static_cast<uint8_t*>(fa.slot[p]), src, bytes,
             (blockIdx.x % wgs_per_peer) * blockDim.x + threadIdx.x,
             static_cast<size_t>(wgs_per_peer) * blockDim.x);
    FusedFinish(fa.ctr[p], fa.ctr_target[p], fa.flag[p], fa.flag_val[p]);
}

template <typename T, ReduceOp OP>
__global__ void FanInReduceKernel(T* __restrict__ dst, size_t n,
                                  FanKernArgs fa, PollArgs ab,
                                  unsigned long long* ctr,
                                  unsigned long long ctr_target) {
    // wait every arrival (thread 0 polls each mailbox under ONE wall-clock
    // bound; abort-aware)
    __shared__ int ok;
    if (threadIdx.x == 0) {
        ok = 1;
        const unsigned long long t0 = wall_clock64();
        for (int p = 0; p < fa.npeers && ok; ++p)
            if (!SpinGeq(fa.wait_mbox[p], fa.wait_target[p], ab, t0)) ok = 0;
        // ONE system-scope acquire fence after the relaxed loads that saw
        // every peer's release synchronises with all of them (an acquire
        // per mailbox would cost a cache invalidate each).
        if (ok) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    }
    __syncthreads();
    if (!ok) return;
    const size_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = gridDim.x * blockDim.x;
    for (size_t j = tid; j < n; j += stride) {
        // accumulate in the arithmetic type; bf16 rounds once at the end
        ArithT<T> acc = Decode(dst[j]);
        for (int p = 0; p < fa.npeers; ++p)
            acc = Apply<ArithT<T>, OP>(acc, Decode(static_cast<const T*>(fa.slot[p])[j]));
        dst[j] = Encode<T>(acc);
    }
    // single counter; the finisher publishes every ack
    FusedFinish(ctr, ctr_target, fa.flag, fa.flag_val, fa.npeers);
}

FanKernArgs ToKernArgs(const FanPeer* peers, int np) {
    FanKernArgs fa{};
    fa.npeers = np;
    for (int p = 0; p < np; ++p) {
        fa.slot[p] = peers[p].slot;
        fa.flag[p] = U64(peers[p].flag);
        fa.flag_val[p] = peers[p].flag_val;
        fa.wait_mbox[p] =
            static_cast<const unsigned long long*>(peers[p].wait_mbox);
        fa.wait_target[p] = peers[p].wait_target;
        fa.ctr[p] = U64(peers[p].ctr);
        fa.ctr_target[p] = peers[p].ctr_target;
    }
    return fa;
}

}  // namespace

int FanOutWgsPerPeer(int npeers) {
    // Total spinner budget ~32 wgs per launch: one peer gets the full
    // bandwidth grid, many peers split it (>= 4 each).
    if (npeers <= 1) return 32;
    if (npeers <= 4) return 8;
    return 4;
}

void LaunchFanOutSend(const void* src, size_t bytes, const FanPeer* peers,
                      int npeers, const XferPoll* ab, hipStream_t stream) {
    const int wpp = FanOutWgsPerPeer(npeers);
    FanOutSendKernel<<<dim3(wpp * npeers), dim3(kBlock), 0, stream>>>(
        static_cast<const uint8_t*>(src), bytes, ToKernArgs(peers, npeers),
        ToPollArgs(ab), wpp);
    HIP_CHECK(hipGetLastError());
}

bool LaunchFanInReduce(void* dst, size_t n, DataType dt, ReduceOp op,
                       const FanPeer* peers, int npeers, void* ctr,
                       uint64_t ctr_target, const XferPoll* ab,
                       hipStream_t stream) {
    if (dt != DataType::F32 && dt != DataType::BF16) return false;
    const FanKernArgs fa = ToKernArgs(peers, npeers);
    const PollArgs pa = ToPollArgs(ab);
    DispatchOp(op, [&](auto o) {
        auto launch = [&](auto* typed_dst) {
            using T = std::remove_pointer_t<decltype(typed_dst)>;
            FanInReduceKernel<T, decltype(o)::value>
                <<<dim3(kXferFusedGrid), dim3(kBlock), 0, stream>>>(
                    typed_dst, n, fa, pa, U64(ctr), ctr_target);
        };
        if (dt == DataType::F32) launch(static_cast<float*>(dst));
        else launch(static_cast<unsigned short*>(dst));
    });
    HIP_CHECK(hipGetLastError());
    return true;
}

void LaunchWaitFlag(const void* mbox, uint64_t target, const void* abort_word,
                    void* status, uint64_t max_ticks, hipStream_t stream) {
    const XferPoll poll{mbox, target, abort_word, status, max_ticks};
    WaitFlagKernel<<<dim3(1), dim3(1), 0, stream>>>(ToPollArgs(&poll));
    HIP_CHECK(hipGetLastError());
}

void LaunchSetFlag(void* mbox, uint64_t val, hipStream_t stream) {
    SetFlagKernel<<<dim3(1), dim3(1), 0, stream>>>(U64(mbox), val);
    HIP_CHECK(hipGetLastError());
}

}  // namespace mlsl
