// Types and kernels around the flash-attention prefill kernels (ops_flash.hip: bf16 / f16 products; ops_flash_fp8.hip: e4m3
// first product): MFMA / packing wrappers (also used by the conv and audio kernels), the policies, the V^T image and its
// transposing pre-pass, the KV split and its merge kernel.  The kernels' shared tile walk is flash_core.hip.h.
#pragma once

#include <type_traits>

#include "attn_plan.h"
#include "pgk_device.hip.h"

namespace pgk {

typedef __bf16 bf16x8_fl __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8_fl __attribute__((ext_vector_type(8)));
typedef float f32x16_fl __attribute__((ext_vector_type(16)));

template <class T> __device__ __forceinline__ f32x16_fl mfma32(const uint4& a, const uint4& b, f32x16_fl c);
template <> __device__ __forceinline__ f32x16_fl mfma32<bf16>(const uint4& a, const uint4& b, f32x16_fl c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_fl, a), __builtin_bit_cast(bf16x8_fl, b), c, 0, 0, 0);
}
template <> __device__ __forceinline__ f32x16_fl mfma32<f16>(const uint4& a, const uint4& b, f32x16_fl c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_fl, a), __builtin_bit_cast(f16x8_fl, b), c, 0, 0, 0);
}
template <class T> __device__ __forceinline__ uint32_t pack16x2(float lo, float hi);
template <> __device__ __forceinline__ uint32_t pack16x2<bf16>(float lo, float hi) { return pack_bf16x2(lo, hi); }
template <> __device__ __forceinline__ uint32_t pack16x2<f16>(float lo, float hi) {
    return (uint32_t)__builtin_bit_cast(uint16_t, static_cast<_Float16>(lo)) | ((uint32_t)__builtin_bit_cast(uint16_t, static_cast<_Float16>(hi)) << 16);
}

// Optional last argument of flash_fwd_kernel (ops_flash.hip).  FlashPlain: sdpa_causal, mask offset kv_len - q_len, one
// scale for every row.  FlashIrope: sdpa_irope (ops_llama4.hip), the row's temperature folded into the Q premultiply and
// a free mask offset.  FlashAlibi: sdpa_alibi (ops_posenc.hip), mask as FlashPlain, the score of (row i, key j) of query head h
// gets -slopes[h] * (kv_len - q_len + i - j): the MFMA accumulators of Q.K^T start at that bias instead of at zero.
// FlashFull: sdpa_noncausal (ops_attention.hip), every key visible to every query row, kv_len and q_len unrelated.
// FlashRelBias: sdpa_relbias (ops_relbias.hip), FlashFull's mask and a per-head table of biases by key - query distance (below).
struct FlashPlain {};
struct FlashFull {};        // sdpa_noncausal: no mask but the end of the keys (mask offset kv_len)
struct FlashIrope {
    const void* positions;   // [q_len] int64 or int32
    float attn_scale, floor_scale;
    int causal_offset;       // row i sees kv j <= i + causal_offset
    int pos_is_i64;
};
struct FlashAlibi {
    const float* slopes;     // [Hq] fp32, one per QUERY head
};
// sdpa_relbias (ops_relbias.hip): no mask, as FlashFull; the score of (row i, key j) of query head h gets
// table[h][clamp(j - i, -radius, radius) + radius] (T5's bucketed relative-position bias, folded to one entry per delta).  The
// head's row is staged into LDS once per workgroup - in the exp2 domain, padded on both sides by FL_RELBIAS_PAD copies of the
// saturated entries - and the accumulators of Q.K^T start from it (attn_plan.h: relbias_tile_class).
struct FlashRelBias {
    const float* table;      // [Hq][2 * radius + 1] fp32, one row per QUERY head
    int radius;              // 0 .. FL_RELBIAS_MAX_RADIUS
};

// V^T image: [D][64 kv] 16-bit = 128-byte rows, 8-byte chunk c8 (0..15) of row d at d*128 + ((c8 ^ ((d>>1) & 15)) << 3):
// the 32 rows a half-wave reads at one c8 then fall on 32 different bank pairs
__device__ __forceinline__ int fl_v_off(int d, int c8) { return d * 128 + ((c8 ^ ((d >> 1) & 15)) << 3); }

// KV split (short prompts): nsplit > 1 cuts a query tile's KV tiles into nsplit contiguous runs, one workgroup each; every
// workgroup leaves a NORMALISED partial output (type T) and its (m, l) per row, and flash_merge_kernel combines them.
// Without it the causal imbalance sets the time of a short prompt: at S = 2048 with 16 heads there are 256 workgroups -
// one per CU, the heaviest walks 32 KV tiles, the lightest 2 - and the launch lasts as long as the heaviest (52 us for
// 17 GFLOP).  Cut in two and dealt heavy-first, two half-runs share a CU and the CUs finish together.
struct FlashSplit {
    int nsplit;
    float* ml;      // [nsplit][Hq][q_len][2]  (m in the exp2 domain, l)
    void* o;        // [nsplit][q_len][Hq][D] of T
    // fp8 x fp8 prefill (D = 128, bf16): instead of out, e4m3 codes [q_len][Hq * D] and one scale per (row, head) [q_len][Hq]
    // - a head's 128 output dims ARE one 128-wide scale block of the o_proj's A operand (quantize_fp8_rows' contract:
    // scale = absmax / 448 of the bf16-rounded values, 1 for an all-zero block), written by whichever kernel holds the final
    // row: this one (nsplit == 1) or flash_merge_kernel
    uint8_t* q8;
    float* q8s;
};

// out[q][head][:] = sum_s w_s o_s / sum_s w_s,  w_s = l_s 2^(m_s - max m): one thread per 8 output elements
template <class T, int D>
__global__ __launch_bounds__(256) void flash_merge_kernel(const float* ml, const T* po, T* out, int hq, int q_len, int nsplit, long long oh, long long os,
                                                          uint8_t* q8 = nullptr, float* q8s = nullptr) {
    constexpr int CPR = D / 8;
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t nrow = (size_t)q_len * hq;
    if (gid >= nrow * CPR) return;          // nrow * CPR is a multiple of 16: the 16 lanes of a (row, head) stay together
    const size_t rowi = gid / CPR;
    const int c = (int)(gid % CPR), qrow = (int)(rowi / hq), head = (int)(rowi % hq);
    float mstar = -INFINITY;
    for (int s2 = 0; s2 < nsplit; ++s2) mstar = fmaxf(mstar, ml[(((size_t)s2 * hq + head) * q_len + qrow) * 2]);
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, den = 0.f;
    for (int s2 = 0; s2 < nsplit; ++s2) {
        const float* r = ml + (((size_t)s2 * hq + head) * q_len + qrow) * 2;
        const float w = (r[1] > 0.f) ? r[1] * __builtin_amdgcn_exp2f(r[0] - mstar) : 0.f;
        if (w > 0.f) {
            Vec<T> v;
            v.load(po + (((size_t)s2 * q_len + qrow) * hq + head) * D + c * 8);
            float f[8];
            v.to_float(f);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = fmaf(w, f[j], acc[j]);
            den += w;
        }
    }
    const float inv = den > 0.f ? 1.f / den : 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] *= inv;
    Vec<T> v;
    v.from_float(acc);
    if constexpr (std::is_same<T, bf16>::value && D == 128) {
        if (q8 != nullptr) {                // see FlashSplit::q8: 16 lanes x 8 dims = one (row, head) = one scale block
            v.to_float(acc);
            float amax = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(acc[j]));
            amax = group16_max(amax);
            const float sc = amax > 0.f ? amax / 448.0f : 1.0f;
            uint2 o8;
            o8.x = pack_fp8x4(acc[0] / sc, acc[1] / sc, acc[2] / sc, acc[3] / sc);
            o8.y = pack_fp8x4(acc[4] / sc, acc[5] / sc, acc[6] / sc, acc[7] / sc);
            *reinterpret_cast<uint2*>(q8 + rowi * D + c * 8) = o8;
            if (c == 0) q8s[rowi] = sc;
            return;
        }
    }
    v.store(out + (size_t)head * oh + (size_t)qrow * os + c * 8);
}

// V [Hkv][kv][D] (element strides kh, ks) -> V^T [Hkv][D][kv_pad], zero beyond kv_len.  One workgroup per
// (64-position tile, kv head); the tile goes through LDS so both sides move 16-byte chunks.
template <class T, int D>
__global__ __launch_bounds__(256) void transpose_v_kernel(const T* v, T* vt, int kv_len, int kv_pad, long long kh, long long ks) {
    __shared__ uint16_t tile[64][D + 2];
    const int kv0 = blockIdx.x * 64, head = blockIdx.y;
    const T* vh = v + (size_t)head * kh;
    constexpr int NC = D / 8;
    for (int c = threadIdx.x; c < 64 * NC; c += 256) {
        const int r = c / NC, kc = c % NC;
        uint4 x = make_uint4(0, 0, 0, 0);
        if (kv0 + r < kv_len) x = *reinterpret_cast<const uint4*>(vh + (size_t)(kv0 + r) * ks + kc * 8);
        const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            tile[r][kc * 8 + 2 * j] = (uint16_t)(w[j] & 0xFFFFu);
            tile[r][kc * 8 + 2 * j + 1] = (uint16_t)(w[j] >> 16);
        }
    }
    __syncthreads();
    T* oh = vt + (size_t)head * D * kv_pad;
    for (int c = threadIdx.x; c < D * 8; c += 256) {
        const int d = c >> 3, kc = c & 7;
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = (uint32_t)tile[kc * 8 + 2 * j][d] | ((uint32_t)tile[kc * 8 + 2 * j + 1][d] << 16);
        *reinterpret_cast<uint4*>(oh + (size_t)d * kv_pad + kv0 + kc * 8) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

}  // namespace pgk
