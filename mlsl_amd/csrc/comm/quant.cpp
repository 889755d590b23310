#include "quant.hpp"

#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../core/log.hpp"

namespace mlsl {

namespace {

inline float Bf16F(uint16_t h) {
    uint32_t u = static_cast<uint32_t>(h) << 16;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

inline uint16_t F32B(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    uint32_t lsb = (u >> 16) & 1;
    u += 0x7fffu + lsb;
    return static_cast<uint16_t>(u >> 16);
}

// Wire block: kWireHdr header bytes ([f32 scale][f32 0]) and the payload.
constexpr size_t kWireHdr = 8;
// The N-way kernels take their wires by value: at most this many.
constexpr int kMaxSumWires = 8;

// The requantizing half of the codec, shared by every function that writes a
// wire block (the device side is QScale / QRound in hip/kernels.hip).
inline float BlockScale(float block_max) { return block_max > 0.f ? block_max / 127.f : 1.f; }
inline float QuantRound(float v, float inv_scale) {
    return std::min(127.f, std::max(-127.f, std::nearbyint(v * inv_scale)));
}

template <typename LOAD, typename STORE>
void QuantizeImpl(LOAD load, STORE store, void* wire, size_t count, size_t block,
                  bool use_err) {
    const size_t nblocks = (count + block - 1) / block;
    uint8_t* w = static_cast<uint8_t*>(wire);
    for (size_t b = 0; b < nblocks; ++b) {
        const size_t base = b * block;
        const size_t n = std::min(block, count - base);
        uint8_t* wb = w + b * (block + 8);
        float* hdr = reinterpret_cast<float*>(wb);
        int8_t* payload = reinterpret_cast<int8_t*>(wb + 8);
        float m = 0.f;
        for (size_t i = 0; i < n; ++i) m = std::max(m, std::fabs(load(base + i, use_err)));
        const float scale = BlockScale(m);
        hdr[0] = scale;
        hdr[1] = 0.f;
        const float inv = 1.f / scale;
        for (size_t i = 0; i < n; ++i) {
            float v = load(base + i, use_err);
            const float q = QuantRound(v, inv);
            payload[i] = static_cast<int8_t>(q);
            if (use_err) store(base + i, v - q * scale);
        }
        for (size_t i = n; i < block; ++i) payload[i] = 0;
    }
}

}  // namespace

void HostQuantize(const void* in, void* err, void* wire, size_t count, size_t block,
                  DataType dt, bool use_err) {
    if (dt == DataType::F32) {
        const float* p = static_cast<const float*>(in);
        float* e = static_cast<float*>(err);
        QuantizeImpl(
            [&](size_t i, bool ue) { return ue ? p[i] + e[i] : p[i]; },
            [&](size_t i, float v) { e[i] = v; }, wire, count, block, use_err);
    } else if (dt == DataType::BF16) {
        const uint16_t* p = static_cast<const uint16_t*>(in);
        uint16_t* e = static_cast<uint16_t*>(err);
        QuantizeImpl(
            [&](size_t i, bool ue) { return ue ? Bf16F(p[i]) + Bf16F(e[i]) : Bf16F(p[i]); },
            [&](size_t i, float v) { e[i] = F32B(v); }, wire, count, block, use_err);
    } else {
        MLSL_THROW("quantization supports f32/bf16 only");
    }
}

void HostDequantize(const void* wire, void* out, size_t count, size_t block, DataType dt) {
    const size_t nblocks = (count + block - 1) / block;
    const uint8_t* w = static_cast<const uint8_t*>(wire);
    for (size_t b = 0; b < nblocks; ++b) {
        const size_t base = b * block;
        const size_t n = std::min(block, count - base);
        const uint8_t* wb = w + b * (block + 8);
        const float scale = reinterpret_cast<const float*>(wb)[0];
        const int8_t* payload = reinterpret_cast<const int8_t*>(wb + 8);
        if (dt == DataType::F32) {
            float* o = static_cast<float*>(out);
            for (size_t i = 0; i < n; ++i) o[base + i] = payload[i] * scale;
        } else if (dt == DataType::BF16) {
            uint16_t* o = static_cast<uint16_t*>(out);
            for (size_t i = 0; i < n; ++i) o[base + i] = F32B(payload[i] * scale);
        } else {
            MLSL_THROW("dequantization supports f32/bf16 only");
        }
    }
}

void HostQuantAccum(void* acc_wire, const void* wire, size_t count, size_t block) {
    const size_t nblocks = (count + block - 1) / block;
    uint8_t* aw = static_cast<uint8_t*>(acc_wire);
    const uint8_t* iw = static_cast<const uint8_t*>(wire);
    for (size_t b = 0; b < nblocks; ++b) {
        const size_t base = b * block;
        const size_t n = std::min(block, count - base);
        uint8_t* ab = aw + b * (block + 8);
        const uint8_t* ib = iw + b * (block + 8);
        float* ahdr = reinterpret_cast<float*>(ab);
        const float as = ahdr[0];
        const float is = reinterpret_cast<const float*>(ib)[0];
        int8_t* ap = reinterpret_cast<int8_t*>(ab + 8);
        const int8_t* ip = reinterpret_cast<const int8_t*>(ib + 8);
        float m = 0.f;
        for (size_t i = 0; i < n; ++i)
            m = std::max(m, std::fabs(ap[i] * as + ip[i] * is));
        const float ns = m > 0.f ? m / 127.f : 1.f;
        const float inv = 1.f / ns;
        for (size_t i = 0; i < n; ++i) {
            float v = ap[i] * as + ip[i] * is;
            float q = std::nearbyint(v * inv);
            ap[i] = static_cast<int8_t>(std::min(127.f, std::max(-127.f, q)));
        }
        ahdr[0] = ns;
    }
}

void HostQuantSumDequant(const void* a_wire, const void* b_wire, void* out,
                         size_t count, size_t block, DataType dt) {
    CheckQuantBlock(block, "HostQuantSumDequant");
    if (dt != DataType::F32 && dt != DataType::BF16)
        MLSL_THROW("quantized sum-dequantize supports f32/bf16 only");
    const size_t nblocks = (count + block - 1) / block;
    const uint8_t* aw = static_cast<const uint8_t*>(a_wire);
    const uint8_t* bw = static_cast<const uint8_t*>(b_wire);
    for (size_t blk = 0; blk < nblocks; ++blk) {
        const size_t base = blk * block;
        const size_t n = std::min(block, count - base);
        const uint8_t* ab = aw + blk * (block + 8);
        const uint8_t* bb = bw + blk * (block + 8);
        const float as = reinterpret_cast<const float*>(ab)[0];
        const float bs = reinterpret_cast<const float*>(bb)[0];
        const int8_t* ap = reinterpret_cast<const int8_t*>(ab + 8);
        const int8_t* bp = reinterpret_cast<const int8_t*>(bb + 8);
        if (dt == DataType::F32) {
            float* o = static_cast<float*>(out);
            for (size_t i = 0; i < n; ++i) o[base + i] = ap[i] * as + bp[i] * bs;
        } else {
            uint16_t* o = static_cast<uint16_t*>(out);
            for (size_t i = 0; i < n; ++i) o[base + i] = F32B(ap[i] * as + bp[i] * bs);
        }
    }
}

void HostQuantSumDequantN(const void* const* wires, int nwires, void* out, size_t count,
                          size_t block, DataType dt) {
    CheckQuantBlock(block, "HostQuantSumDequantN");
    if (dt != DataType::F32 && dt != DataType::BF16)
        MLSL_THROW("quantized sum-dequantize supports f32/bf16 only");
    MLSL_CHECK(nwires >= 1 && nwires <= 8, "quantized sum-dequantize takes 1 to 8 wires");
    for (int r = 0; r < nwires; ++r)
        MLSL_CHECK(wires[r] != nullptr, "quantized sum-dequantize: null wire");
    const size_t nblocks = (count + block - 1) / block;
    for (size_t blk = 0; blk < nblocks; ++blk) {
        const size_t base = blk * block;
        const size_t n = std::min(block, count - base);
        float s[8];
        const int8_t* p[8];
        for (int r = 0; r < nwires; ++r) {
            const uint8_t* wb = static_cast<const uint8_t*>(wires[r]) + blk * (block + 8);
            std::memcpy(&s[r], wb, 4);
            p[r] = reinterpret_cast<const int8_t*>(wb + 8);
        }
        for (size_t i = 0; i < n; ++i) {
            // wire order, one explicit fma per wire: the device kernel's bits
            float acc = 0.f;
            for (int r = 0; r < nwires; ++r)
                acc = std::fmaf(static_cast<float>(p[r][i]), s[r], acc);
            if (dt == DataType::F32) static_cast<float*>(out)[base + i] = acc;
            else static_cast<uint16_t*>(out)[base + i] = F32B(acc);
        }
    }
}

void HostQuantSumRequantN(const void* const* wires, int nwires, void* dst_wire,
                          size_t nunits, size_t block) {
    CheckQuantBlock(block, "HostQuantSumRequantN");
    MLSL_CHECK(nwires >= 1 && nwires <= kMaxSumWires,
               "quantized sum-requantize takes 1 to 8 wires");
    MLSL_CHECK(dst_wire != nullptr, "quantized sum-requantize: null destination");
    for (int r = 0; r < nwires; ++r)
        MLSL_CHECK(wires[r] != nullptr, "quantized sum-requantize: null wire");
    // a unit's sums are complete before its first byte is written, so dst_wire
    // may be one of the wires
    std::vector<float> acc(block);
    for (size_t blk = 0; blk < nunits; ++blk) {
        float s[kMaxSumWires];
        const int8_t* p[kMaxSumWires];
        for (int r = 0; r < nwires; ++r) {
            const uint8_t* wb = static_cast<const uint8_t*>(wires[r]) + blk * (block + kWireHdr);
            std::memcpy(&s[r], wb, 4);
            p[r] = reinterpret_cast<const int8_t*>(wb + kWireHdr);
        }
        float m = 0.f;
        for (size_t i = 0; i < block; ++i) {
            // wire order, one explicit fma per wire: the device kernel's bits
            float a = 0.f;
            for (int r = 0; r < nwires; ++r)
                a = std::fmaf(static_cast<float>(p[r][i]), s[r], a);
            acc[i] = a;
            m = std::max(m, std::fabs(a));
        }
        const float scale = BlockScale(m);
        const float inv = 1.f / scale;
        uint8_t* db = static_cast<uint8_t*>(dst_wire) + blk * (block + kWireHdr);
        int8_t* dp = reinterpret_cast<int8_t*>(db + kWireHdr);
        for (size_t i = 0; i < block; ++i) dp[i] = static_cast<int8_t>(QuantRound(acc[i], inv));
        const float hdr[2] = {scale, 0.f};
        std::memcpy(db, hdr, kWireHdr);
    }
}

void HostDequantizeSegments(const void* wire, size_t nseg, void* out, size_t count,
                            size_t block, DataType dt, bool accumulate) {
    CheckQuantBlock(block, "HostDequantizeSegments");
    if (dt != DataType::F32 && dt != DataType::BF16)
        MLSL_THROW("segmented dequantize supports f32/bf16 only");
    MLSL_CHECK(nseg >= 1, "segmented dequantize takes at least one segment");
    const size_t nblocks = (count + block - 1) / block;
    const size_t seg_wire = nblocks * (block + 8);
    for (size_t seg = 0; seg < nseg; ++seg) {
        // every segment has a block grid of its own: a partial last block is
        // followed by the next segment's block 0, not by the rest of a block
        const uint8_t* w = static_cast<const uint8_t*>(wire) + seg * seg_wire;
        for (size_t blk = 0; blk < nblocks; ++blk) {
            const size_t base = seg * count + blk * block;
            const size_t n = std::min(block, count - blk * block);
            const uint8_t* wb = w + blk * (block + 8);
            float s;
            std::memcpy(&s, wb, 4);
            const int8_t* p = reinterpret_cast<const int8_t*>(wb + 8);
            for (size_t i = 0; i < n; ++i) {
                const float q = static_cast<float>(p[i]);
                if (dt == DataType::F32) {
                    float* o = static_cast<float*>(out) + base + i;
                    *o = accumulate ? std::fmaf(q, s, *o) : q * s;
                } else {
                    uint16_t* o = static_cast<uint16_t*>(out) + base + i;
                    *o = F32B(accumulate ? std::fmaf(q, s, Bf16F(*o)) : q * s);
                }
            }
        }
    }
}

namespace {

// Element idx of the concatenation -> its tensor: a cursor that walks the
// prefix table either way, so the sequential passes of the codec cost one
// step per boundary crossed.
struct SegCursor {
    const uint64_t* offs;
    size_t nseg;
    size_t s = 0;
    // (tensor, element in it) of idx < offs[nseg]
    size_t Seek(size_t idx) {
        while (idx < offs[s]) --s;
        while (s + 1 < nseg && idx >= offs[s + 1]) ++s;
        return idx - offs[s];
    }
};

void CheckSegTables(const void* ptrs, const uint64_t* offs, size_t nseg, size_t count,
                    DataType dt, const char* where) {
    if (dt != DataType::F32 && dt != DataType::BF16)
        MLSL_THROW(std::string(where) + " supports f32/bf16 only");
    MLSL_CHECK(nseg >= 1, std::string(where) + " takes at least one segment");
    MLSL_CHECK(ptrs != nullptr && offs != nullptr, std::string(where) + ": null segment table");
    MLSL_CHECK(offs[0] == 0 && offs[nseg] == count,
               std::string(where) + ": offsets do not run from 0 to count");
    for (size_t j = 0; j < nseg; ++j)
        MLSL_CHECK(offs[j + 1] > offs[j],
                   std::string(where) + ": segment " + std::to_string(j) + " is empty");
}

}  // namespace

void HostQuantizeGather(const void* const* seg_ptrs, const uint64_t* seg_offs, size_t nseg,
                        void* err, void* wire, size_t count, size_t block, DataType dt,
                        bool use_err) {
    CheckQuantBlock(block, "HostQuantizeGather");
    CheckSegTables(seg_ptrs, seg_offs, nseg, count, dt, "quantize-gather");
    SegCursor cur{seg_offs, nseg};
    // HostQuantize's two instantiations, reading through the cursor
    if (dt == DataType::F32) {
        float* e = static_cast<float*>(err);
        auto in = [&](size_t i) {
            const size_t k = cur.Seek(i);
            return static_cast<const float*>(seg_ptrs[cur.s])[k];
        };
        QuantizeImpl([&](size_t i, bool ue) { return ue ? in(i) + e[i] : in(i); },
                     [&](size_t i, float v) { e[i] = v; }, wire, count, block, use_err);
    } else {
        uint16_t* e = static_cast<uint16_t*>(err);
        auto in = [&](size_t i) {
            const size_t k = cur.Seek(i);
            return Bf16F(static_cast<const uint16_t*>(seg_ptrs[cur.s])[k]);
        };
        QuantizeImpl([&](size_t i, bool ue) { return ue ? in(i) + Bf16F(e[i]) : in(i); },
                     [&](size_t i, float v) { e[i] = F32B(v); }, wire, count, block, use_err);
    }
}

void HostQuantizeGatherShards(const void* const* seg_ptrs, const uint64_t* seg_offs,
                              size_t nseg, void* err, void* wire, size_t total,
                              size_t nshards, size_t shard, size_t wire_stride, size_t block,
                              DataType dt, bool use_err) {
    CheckQuantBlock(block, "HostQuantizeGatherShards");
    CheckSegTables(seg_ptrs, seg_offs, nseg, total, dt, "quantize-gather-shards");
    MLSL_CHECK(nshards >= 1 && shard >= (total + nshards - 1) / nshards,
               "quantize-gather-shards: shard * nshards < total (the shards do not hold "
               "the tensors)");
    MLSL_CHECK(wire_stride % 4 == 0 &&
                   wire_stride >= (shard + block - 1) / block * (block + kWireHdr),
               "quantize-gather-shards: wire_stride is smaller than one shard's wire or "
               "no multiple of 4");
    MLSL_CHECK(!use_err || err != nullptr, "quantize-gather-shards: use_err without err");
    SegCursor cur{seg_offs, nseg};
    // HostQuantize of every shard of V', reading through the cursor; an element
    // at or past `total` is 0, and neither a tensor nor the residual is touched
    // for it
    for (size_t j = 0; j < nshards; ++j) {
        const size_t lo = j * shard;
        uint8_t* w = static_cast<uint8_t*>(wire) + j * wire_stride;
        if (dt == DataType::F32) {
            float* e = static_cast<float*>(err);
            auto in = [&](size_t i) {
                const size_t k = cur.Seek(i);
                return static_cast<const float*>(seg_ptrs[cur.s])[k];
            };
            QuantizeImpl(
                [&](size_t i, bool ue) {
                    i += lo;
                    return i >= total ? 0.f : ue ? in(i) + e[i] : in(i);
                },
                [&](size_t i, float v) { if (i + lo < total) e[i + lo] = v; }, w, shard,
                block, use_err);
        } else {
            uint16_t* e = static_cast<uint16_t*>(err);
            auto in = [&](size_t i) {
                const size_t k = cur.Seek(i);
                return Bf16F(static_cast<const uint16_t*>(seg_ptrs[cur.s])[k]);
            };
            QuantizeImpl(
                [&](size_t i, bool ue) {
                    i += lo;
                    return i >= total ? 0.f : ue ? in(i) + Bf16F(e[i]) : in(i);
                },
                [&](size_t i, float v) { if (i + lo < total) e[i + lo] = F32B(v); }, w, shard,
                block, use_err);
        }
    }
}

void HostDequantizeScatter(const void* wire, void* const* seg_ptrs, const uint64_t* seg_offs,
                           size_t nseg, size_t count, size_t block, DataType dt,
                           float post_scale, bool round_first) {
    CheckQuantBlock(block, "HostDequantizeScatter");
    const bool pre_round = round_first && dt == DataType::BF16;
    CheckSegTables(seg_ptrs, seg_offs, nseg, count, dt, "dequantize-scatter");
    SegCursor cur{seg_offs, nseg};
    const size_t nblocks = (count + block - 1) / block;
    const uint8_t* w = static_cast<const uint8_t*>(wire);
    for (size_t b = 0; b < nblocks; ++b) {
        const size_t base = b * block;
        const size_t n = std::min(block, count - base);
        const uint8_t* wb = w + b * (block + kWireHdr);
        float scale;
        std::memcpy(&scale, wb, 4);
        const int8_t* payload = reinterpret_cast<const int8_t*>(wb + kWireHdr);
        for (size_t i = 0; i < n; ++i) {
            const size_t k = cur.Seek(base + i);
            // two roundings to float, as the device kernel: never one product
            // with scale * post_scale
            float dq = payload[i] * scale;
            if (pre_round) dq = Bf16F(F32B(dq));
            const float v = dq * post_scale;
            if (dt == DataType::F32) static_cast<float*>(seg_ptrs[cur.s])[k] = v;
            else static_cast<uint16_t*>(seg_ptrs[cur.s])[k] = F32B(v);
        }
    }
}

const QuantPluginApi* LoadQuantPlugin(const QuantParams& qp) {
    if (qp.lib_path.empty()) return nullptr;
    static std::mutex mu;
    static std::unordered_map<std::string, QuantPluginApi> cache;
    std::lock_guard<std::mutex> lk(mu);
    const std::string key = qp.lib_path + "|" + qp.quant_fn;
    auto it = cache.find(key);
    if (it != cache.end()) return &it->second;

    void* h = dlopen(qp.lib_path.c_str(), RTLD_NOW);
    if (!h) MLSL_THROW(std::string("quant plugin dlopen failed: ") + dlerror());
    QuantPluginApi api{};
    api.quant = reinterpret_cast<decltype(api.quant)>(dlsym(h, qp.quant_fn.c_str()));
    api.dequant =
        reinterpret_cast<decltype(api.dequant)>(dlsym(h, qp.dequant_fn.c_str()));
    api.reduce_sum = reinterpret_cast<decltype(api.reduce_sum)>(
        dlsym(h, qp.reduce_fn.c_str()));
    if (!api.quant || !api.dequant || !api.reduce_sum)
        MLSL_THROW("quant plugin missing symbol(s): " + qp.quant_fn + "/" +
                   qp.dequant_fn + "/" + qp.reduce_fn);
    MLSL_LOG(INFO, "quant plugin loaded: %s (host path; device path keeps "
             "built-in CDNA4 kernels)", qp.lib_path.c_str());
    return &cache.emplace(key, api).first->second;
}

}  // namespace mlsl
