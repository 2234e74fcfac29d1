// Weight-streaming GEMV core for gfx950, shared by the op-level GEMV (ops_gemv.hip) and
// the fused decode kernels (engine_gemv.hip.h).
//
//   y[m][n] = sum_k x[m][k] * W[n][k]        W is [N,K] row-major (PyTorch [out,in]), M small.
//
// Design (wave64, HBM-bound):
//   * the activation rows x[M][K] are staged ONCE per workgroup in LDS; weights are read
//     exactly once from HBM, straight to VGPRs (no LDS round trip for a read-once operand),
//     16 bytes per lane = 1 KiB per wave-instruction, fully coalesced along K, non-temporal;
//   * one wave owns R consecutive output rows at a time: R independent 16-B loads in flight
//     per lane per k-step, and one LDS read of the x fragment is reused by the R rows;
//   * fp32 accumulation; cross-lane reduction by 6 xor-shuffles per output.
// The reference's kernel (native/ops/matmul/gemv/bf16_bf16/sm120/bf16_opt.cuh:56-231) is
// "one 32-lane warp per output row, A in shared memory"; this is a re-derivation for
// 64-lane waves, not a transliteration.
#pragma once

#include <type_traits>

#include "pgk_device.hip.h"

namespace pgk {

struct fp8e4m3 { uint8_t b; };

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint4 load_nt16(const void* p) {
    const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}

// ---- 16 bytes of weights -> NW floats -----------------------------------------------------
template <class WT> struct WTraits;
template <> struct WTraits<bf16> {
    static constexpr int NW = 8;
    __device__ static __forceinline__ void decode(const uint4& r, float (&f)[8]) {
        const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f[2 * i] = __uint_as_float(w[i] << 16);
            f[2 * i + 1] = __uint_as_float(w[i] & 0xFFFF0000u);
        }
    }
};
template <> struct WTraits<f16> {
    static constexpr int NW = 8;
    __device__ static __forceinline__ void decode(const uint4& r, float (&f)[8]) {
        Vec<f16> v;
        v.raw = r;
        v.to_float(f);
    }
};
template <> struct WTraits<float> {
    static constexpr int NW = 4;
    __device__ static __forceinline__ void decode(const uint4& r, float (&f)[4]) {
        f[0] = __uint_as_float(r.x); f[1] = __uint_as_float(r.y);
        f[2] = __uint_as_float(r.z); f[3] = __uint_as_float(r.w);
    }
};
// OCP e4m3 (gfx950's native fp8; MI300's fnuz is a different encoding): v_cvt_pk_f32_fp8.
template <> struct WTraits<fp8e4m3> {
    static constexpr int NW = 16;
    __device__ static __forceinline__ void decode(const uint4& r, float (&f)[16]) {
        const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
            const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
            f[4 * i] = lo.x; f[4 * i + 1] = lo.y; f[4 * i + 2] = hi.x; f[4 * i + 3] = hi.y;
        }
    }
};

// ---- NW consecutive activations from LDS -> floats ----------------------------------------
template <class XT, int NW> struct XLoad;
template <int NW> struct XLoad<float, NW> {
    __device__ static __forceinline__ void load(const float* xs, float (&f)[NW]) {
#pragma unroll
        for (int i = 0; i < NW / 4; ++i) {
            const float4 v = *reinterpret_cast<const float4*>(xs + 4 * i);
            f[4 * i] = v.x; f[4 * i + 1] = v.y; f[4 * i + 2] = v.z; f[4 * i + 3] = v.w;
        }
    }
};
template <int NW> struct XLoad<bf16, NW> {
    __device__ static __forceinline__ void load(const bf16* xs, float (&f)[NW]) {
        if constexpr (NW == 4) {
            const uint2 v = *reinterpret_cast<const uint2*>(xs);
            f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xFFFF0000u);
            f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xFFFF0000u);
        } else {
#pragma unroll
            for (int i = 0; i < NW / 8; ++i) {
                float t[8];
                WTraits<bf16>::decode(*reinterpret_cast<const uint4*>(xs + 8 * i), t);
#pragma unroll
                for (int j = 0; j < 8; ++j) f[8 * i + j] = t[j];
            }
        }
    }
};
template <int NW> struct XLoad<f16, NW> {
    __device__ static __forceinline__ void load(const f16* xs, float (&f)[NW]) {
        if constexpr (NW == 4) {
#pragma unroll
            for (int j = 0; j < 4; ++j) f[j] = static_cast<float>(xs[j].v);
        } else {
#pragma unroll
            for (int i = 0; i < NW / 8; ++i) {
                float t[8];
                WTraits<f16>::decode(*reinterpret_cast<const uint4*>(xs + 8 * i), t);
#pragma unroll
                for (int j = 0; j < 8; ++j) f[8 * i + j] = t[j];
            }
        }
    }
};

// bf16 x bf16: v_dot2c_f32_bf16 consumes two packed pairs per instruction (products exact in fp32, fp32
// accumulate) - 4 instructions per 16-byte chunk instead of 8 unpacks + 8 FMAs; this is what keeps the
// M >= 4 batched GEMV from going VALU-bound.
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float dot8_bf16(const uint4& w, const uint4& x, float acc) {
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, w.x), __builtin_bit_cast(bf16x2_t, x.x), acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, w.y), __builtin_bit_cast(bf16x2_t, x.y), acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, w.z), __builtin_bit_cast(bf16x2_t, x.z), acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, w.w), __builtin_bit_cast(bf16x2_t, x.w), acc, false);
    return acc;
}

// Partial dot products of R weight rows against M activation rows over the K range this lane
// owns (k = lane*NW + i*64*NW).  wrow[r] points at row r's first element; xs is x[M][ldx] in LDS.
// Results are per-lane partials: the caller reduces across the wave.
template <class WT, class XT, int M, int R>
__device__ __forceinline__ void gemv_rows(const WT* const (&wrow)[R], const XT* xs, int ldx, int K, int lane,
                                          float (&acc)[R][M]) {
    constexpr int NW = WTraits<WT>::NW;
    if constexpr (std::is_same<WT, bf16>::value && std::is_same<XT, bf16>::value) {
#pragma unroll 2
        for (int k0 = lane * 8; k0 < K; k0 += 64 * 8) {
            uint4 raw[R], xr[M];
#pragma unroll
            for (int r = 0; r < R; ++r) raw[r] = load_nt16(wrow[r] + k0);
#pragma unroll
            for (int m = 0; m < M; ++m) xr[m] = *reinterpret_cast<const uint4*>(xs + (size_t)m * ldx + k0);
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int m = 0; m < M; ++m) acc[r][m] = dot8_bf16(raw[r], xr[m], acc[r][m]);
        }
        return;
    }
#pragma unroll 2
    for (int k0 = lane * NW; k0 < K; k0 += 64 * NW) {
        uint4 raw[R];
#pragma unroll
        for (int r = 0; r < R; ++r) raw[r] = load_nt16(wrow[r] + k0);
        float xf[M][NW];
#pragma unroll
        for (int m = 0; m < M; ++m) XLoad<XT, NW>::load(xs + (size_t)m * ldx + k0, xf[m]);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float wf[NW];
            WTraits<WT>::decode(raw[r], wf);
#pragma unroll
            for (int m = 0; m < M; ++m) {
#pragma unroll
                for (int j = 0; j < NW; ++j) acc[r][m] = fmaf(wf[j], xf[m][j], acc[r][m]);
            }
        }
    }
}

// fp8 variant with one bf16 scale per 128x128 weight block: scale row pointer per weight row,
// index k0/128.  (16 | 128, so a lane's 16 codes never straddle a block.)
template <class XT, int M, int R>
__device__ __forceinline__ void gemv_rows_fp8(const fp8e4m3* const (&wrow)[R], const bf16* const (&srow)[R],
                                              const XT* xs, int ldx, int K, int lane, float (&acc)[R][M]) {
    constexpr int NW = 16;
#pragma unroll 2
    for (int k0 = lane * NW; k0 < K; k0 += 64 * NW) {
        uint4 raw[R];
        float sc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            raw[r] = load_nt16(wrow[r] + k0);
            sc[r] = to_f(srow[r][k0 >> 7]);
        }
        float xf[M][NW];
#pragma unroll
        for (int m = 0; m < M; ++m) XLoad<XT, NW>::load(xs + (size_t)m * ldx + k0, xf[m]);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float wf[NW];
            WTraits<fp8e4m3>::decode(raw[r], wf);
#pragma unroll
            for (int m = 0; m < M; ++m) {
                float p = 0.f;
#pragma unroll
                for (int j = 0; j < NW; ++j) p = fmaf(wf[j], xf[m][j], p);
                acc[r][m] = fmaf(sc[r], p, acc[r][m]);
            }
        }
    }
}

// ---- NVF4 (w4a16): e2m1 codes, one scale byte per 32 k ------------------------------------------------------------
// Engine layout NK: data [N, K/2] (byte j of a row holds k = 2j in its low nibble, 2j+1 in its high nibble) and
// scale [N, K/32].  A lane's 16-byte load is 32 k of one row, so it carries exactly one scale byte.
struct nvf4x2 { uint8_t b; };   // tag type of the engine's NVF4 weights (two codes per byte)
template <> struct WTraits<nvf4x2> { static constexpr int NW = 32; };

// exact decode of a scale byte: exponent field e -> 2^(e-7), mantissa m -> 1 + m/8 (always a normal fp32)
__device__ __forceinline__ float nvf4_scale_value(uint32_t s) {
    return __uint_as_float(((((s >> 3) & 15u) + 120u) << 23) | ((s & 7u) << 20));
}

// byte B of a dword: (k, k+1) at unit scale.  The conversion's scale operand acts as a power of two (an E8M0 MX scale),
// so 1.0 leaves the e2m1 value as it is and the block's scale byte is applied once per 32 k by the caller.
template <int B> __device__ __forceinline__ f32x2 nvf4_pair_f32(uint32_t w) { return __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, B); }
template <int B> __device__ __forceinline__ bf16x2_t nvf4_pair_bf16(uint32_t w) { return __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, 1.0f, B); }

// Activation image in LDS for NVF4 (row m at xs + m * K): a lane owns 32 consecutive k, so reading them in place would
// stride 64 B (bf16) / 128 B (fp32) across the lanes of a ds_read_b128 - 4- / 8-way bank conflicts on every read.  The
// image is stored swizzled instead: k goes to group g = (k % 32) / G (G = 16 bytes of XT), and group g of every 32-k block
// is contiguous, so group g of the wave's 64 blocks is 64 adjacent 16-byte pieces.
template <class XT> __device__ __forceinline__ int nvf4_xpos(int k, int K) {
    constexpr int G = 16 / (int)sizeof(XT), NG = 32 / G;
    return ((k & 31) / G) * (K / NG) + (k >> 5) * G + (k & (G - 1));
}

// p[r][m] += sum over the 32 k of word block k0 of e2m1(raw[r]) * x[m][k]  (unit scale; e2m1 x bf16 products are exact
// in fp32; x is the swizzled image of nvf4_xpos, row stride ldx = K).  bf16 activations: the codes widen to bf16 pairs and v_dot2c_f32_bf16 takes the packed LDS words as they
// are - 2 products per instruction and no unpacking, what keeps M = 4 / 8 from going VALU-bound; fp32 activations
// (M = 1 / 2): fp32 pairs and FMAs.
template <class XT, int M, int R>
__device__ __forceinline__ void nvf4_dot32(const uint4 (&raw)[R], const XT* xs, int ldx, int k0, float (&p)[R][M]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if constexpr (std::is_same<XT, bf16>::value) {
            uint4 xr[M];
#pragma unroll
            for (int m = 0; m < M; ++m) xr[m] = *reinterpret_cast<const uint4*>(xs + (size_t)m * ldx + i * (ldx >> 2) + (k0 >> 5) * 8);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const uint32_t w = i == 0 ? raw[r].x : i == 1 ? raw[r].y : i == 2 ? raw[r].z : raw[r].w;
                const bf16x2_t b0 = nvf4_pair_bf16<0>(w), b1 = nvf4_pair_bf16<1>(w), b2 = nvf4_pair_bf16<2>(w), b3 = nvf4_pair_bf16<3>(w);
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    float t = p[r][m];
                    t = __builtin_amdgcn_fdot2_f32_bf16(b0, __builtin_bit_cast(bf16x2_t, xr[m].x), t, false);
                    t = __builtin_amdgcn_fdot2_f32_bf16(b1, __builtin_bit_cast(bf16x2_t, xr[m].y), t, false);
                    t = __builtin_amdgcn_fdot2_f32_bf16(b2, __builtin_bit_cast(bf16x2_t, xr[m].z), t, false);
                    t = __builtin_amdgcn_fdot2_f32_bf16(b3, __builtin_bit_cast(bf16x2_t, xr[m].w), t, false);
                    p[r][m] = t;
                }
            }
        } else {
            float xf[M][8];
#pragma unroll
            for (int m = 0; m < M; ++m) {
                float lo[4], hi[4];
                XLoad<XT, 4>::load(xs + (size_t)m * ldx + (2 * i) * (ldx >> 3) + (k0 >> 5) * 4, lo);
                XLoad<XT, 4>::load(xs + (size_t)m * ldx + (2 * i + 1) * (ldx >> 3) + (k0 >> 5) * 4, hi);
#pragma unroll
                for (int j = 0; j < 4; ++j) { xf[m][j] = lo[j]; xf[m][4 + j] = hi[j]; }
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const uint32_t w = i == 0 ? raw[r].x : i == 1 ? raw[r].y : i == 2 ? raw[r].z : raw[r].w;
                const f32x2 f0 = nvf4_pair_f32<0>(w), f1 = nvf4_pair_f32<1>(w), f2 = nvf4_pair_f32<2>(w), f3 = nvf4_pair_f32<3>(w);
                const float wf[8] = {f0.x, f0.y, f1.x, f1.y, f2.x, f2.y, f3.x, f3.y};
#pragma unroll
                for (int m = 0; m < M; ++m)
#pragma unroll
                    for (int j = 0; j < 8; ++j) p[r][m] = fmaf(wf[j], xf[m][j], p[r][m]);
            }
        }
    }
}

// NVF4 variant of gemv_rows: wrow[r] = row r's data bytes, srow[r] = its scale bytes; K % 32 == 0.  Each 32-k partial is
// summed at unit scale, then multiplied by its scale byte's value once.
template <class XT, int M, int R>
__device__ __forceinline__ void gemv_rows_nvf4(const uint8_t* const (&wrow)[R], const uint8_t* const (&srow)[R], const XT* xs, int ldx,
                                               int K, int lane, float (&acc)[R][M]) {
    constexpr int NW = 32, UNROLL = M <= 2 ? 2 : 1;   // 4 / 8 activation rows: one trip at a time (registers)
#pragma unroll UNROLL
    for (int k0 = lane * NW; k0 < K; k0 += 64 * NW) {
        uint4 raw[R];
        float sc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            raw[r] = load_nt16(wrow[r] + (k0 >> 1));
            sc[r] = nvf4_scale_value(srow[r][k0 >> 5]);
        }
        float p[R][M];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int m = 0; m < M; ++m) p[r][m] = 0.f;
        nvf4_dot32<XT, M, R>(raw, xs, ldx, k0, p);
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int m = 0; m < M; ++m) acc[r][m] = fmaf(sc[r], p[r][m], acc[r][m]);
    }
}

}  // namespace pgk
