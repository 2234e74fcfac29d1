// NVF4: 4-bit e2m1 values with one byte scale per 32 k (reference: native/ops/matmul/gemv/w4a16_bf16/sm120/
// nvf4.cuh:36-110, nvf4_kernels.cu:19-345 and native/ops/matmul/gemm/w4a16_bf16/sm120/nvf4_cutlass.cu:157-530).
//
//   code c (4 bits): bit 3 = sign, c & 7 indexes {0, .5, 1, 1.5, 2, 3, 4, 6}; a byte holds k (even) in its low
//   nibble and k+1 in its high nibble.
//   weights  data [K/2, N] (byte (k/2)*N + n), scale [ceil(K/32), N] (byte (k/32)*N + n); a scale byte s is
//   (1 + (s&7)/8) * 2^(((s>>3)&15) - 7), bit 7 ignored.
//
// Three kernels:
//   - quantize_nvf4_kernel: bf16 [K,N] -> data + scale, the reference's arithmetic step for step (one thread per
//     (column, 32-row block), coalesced over n);
//   - gemv_nvf4_kernel: C[n] = alpha * sum_kb scale * sum_{k in kb} a[k] * e2m1, weight-streaming (16 columns per lane per
//     dwordx4 load), K split over the 32 k-lanes of a workgroup and, for narrow N, over workgroups; partial sums are
//     added in a fixed order (LDS, then gemv_nvf4_reduce_kernel), so the result does not depend on timing;
//   - gemm_fp4_kernel: the unit-scale GEMM of matmul_nvf4_bf16_sm120 on v_mfma_scale_f32_16x16x128_f8f6f4 with e2m1
//     operands (cbsz = blgp = 4, E8M0 scale 127 = 1.0) over operands packed K-contiguous by quantize_e2m1_kernel.
//
// The quantisers never use the hardware v_cvt_scalef32_pk_fp4_* conversions: those round ties to even (1.25 -> 1)
// where the reference's threshold chains round them away from zero, and bf16 inputs hit those ties exactly.

#include "gemv_core.hip.h"
#include "mfma_common.hip.h"
#include "pgk_internal.h"

namespace pgk {

typedef float f32x2_n __attribute__((ext_vector_type(2)));

// nvf4_scale_value (the exact decode of a scale byte) lives in gemv_core.hip.h, shared with the engine's decode kernels.

// ---- weight quantiser (nvf4_kernels.cu:239-320) ---------------------------------------------------------------

// the reference's `<` chain: ties go away from zero, NaN -> 7 (+6), |v| >= 5 -> 6
__device__ __forceinline__ uint32_t nvf4_code_scaled(float v) {
    const uint32_t sign = v < 0.f ? 8u : 0u;
    const float a = fabsf(v);
    uint32_t c;
    if (a < 0.25f) c = 0;
    else if (a < 0.75f) c = 1;
    else if (a < 1.25f) c = 2;
    else if (a < 1.75f) c = 3;
    else if (a < 2.5f) c = 4;
    else if (a < 3.5f) c = 5;
    else if (a < 5.0f) c = 6;
    else c = 7;
    return sign | c;
}

// the scale byte of a block whose largest magnitude is max_abs (NaN already dropped)
__device__ __forceinline__ uint32_t nvf4_scale_byte(float max_abs) {
    // correctly rounded division (no fast-math in this build): scale = max_abs / 6
    const float s = max_abs > 1e-8f ? max_abs / 6.0f : 1.0f;
    int e = 0;
    float norm = s;
    if (norm >= 2.0f) {
        while (norm >= 2.0f && e < 8) { norm *= 0.5f; ++e; }
    } else if (norm < 1.0f && norm > 1e-8f) {   // the reference's guard: a scale <= 1e-8 is not normalised
        while (norm < 1.0f && e > -7) { norm *= 2.0f; --e; }
    }
    // clamp in float before the conversion: norm = inf (an inf in the block) must give 7, and (int)inf is undefined
    const int mant = (int)fminf(fmaxf(rintf((norm - 1.0f) * 8.0f), 0.f), 7.f);
    const int eb = min(max(e + 7, 0), 15);
    return ((uint32_t)eb << 3) | (uint32_t)mant;
}

__global__ __launch_bounds__(256) void quantize_nvf4_kernel(const bf16* x, uint8_t* data, uint8_t* scale, int K, int N) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int sb = blockIdx.y;
    if (n >= N) return;
    const int k0 = sb * 32, len = min(32, K - k0);   // K is even, so len is too
    float v[32];
    float max_abs = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        v[i] = i < len ? to_f(x[(size_t)(k0 + i) * N + n]) : 0.f;
        max_abs = fmaxf(max_abs, fabsf(v[i]));   // fmaxf drops NaN
    }
    const uint32_t sbyte = nvf4_scale_byte(max_abs);
    scale[(size_t)sb * N + n] = (uint8_t)sbyte;
    const float inv = 1.0f / nvf4_scale_value(sbyte);
#pragma unroll
    for (int i = 0; i < 32; i += 2) {
        if (i < len)
            data[(size_t)((k0 + i) >> 1) * N + n] = (uint8_t)(nvf4_code_scaled(v[i] * inv) | (nvf4_code_scaled(v[i + 1] * inv) << 4));
    }
}

// ---- engine layout NK (ours): data [N, K/2], scale [N, K/32], K % 32 == 0 ---------------------------------------------
// Block i (row i / (K/32), k-block i % (K/32)) is data bytes [16 i, 16 i + 16), scale byte i and bf16 elements
// [32 i, 32 i + 32) of the row-major [N, K] matrix: the three arrays are indexed by the same flat block number.

// The quantiser: the bytes of quantize_nvf4_kernel on x^T, transposed (same block arithmetic, one thread per block).
__global__ __launch_bounds__(256) void quantize_nvf4_nk_kernel(const bf16* x, uint8_t* data, uint8_t* scale, long long nblk) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nblk) return;
    float v[32];
    float max_abs = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float t[8];
        WTraits<bf16>::decode(*reinterpret_cast<const uint4*>(x + i * 32 + 8 * q), t);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            v[8 * q + j] = t[j];
            max_abs = fmaxf(max_abs, fabsf(t[j]));   // fmaxf drops NaN
        }
    }
    const uint32_t sbyte = nvf4_scale_byte(max_abs);
    scale[i] = (uint8_t)sbyte;
    const float inv = 1.0f / nvf4_scale_value(sbyte);
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 32; ++j) w[j >> 3] |= nvf4_code_scaled(v[j] * inv) << (4 * (j & 7));
    *reinterpret_cast<uint4*>(data + i * 16) = make_uint4(w[0], w[1], w[2], w[3]);
}

// bf16 [N, K] = code x scale (exact: an e2m1 value has 2 significant bits, a scale byte 4) - the engine's prefill
// dequantises one layer at a time with this, right before that layer's projections.
__global__ __launch_bounds__(256) void dequant_nvf4_nk_kernel(const uint8_t* data, const uint8_t* scale, bf16* out, long long nblk) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nblk) return;
    const uint4 d = load_nt16(data + i * 16);
    const float s = nvf4_scale_value(scale[i]);
    const uint32_t w[4] = {d.x, d.y, d.z, d.w};
    uint32_t o[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x2 f0 = nvf4_pair_f32<0>(w[q]), f1 = nvf4_pair_f32<1>(w[q]), f2 = nvf4_pair_f32<2>(w[q]), f3 = nvf4_pair_f32<3>(w[q]);
        o[4 * q + 0] = pack_bf16x2(f0.x * s, f0.y * s);
        o[4 * q + 1] = pack_bf16x2(f1.x * s, f1.y * s);
        o[4 * q + 2] = pack_bf16x2(f2.x * s, f2.y * s);
        o[4 * q + 3] = pack_bf16x2(f3.x * s, f3.y * s);
    }
    uint4* dst = reinterpret_cast<uint4*>(out + i * 32);
#pragma unroll
    for (int q = 0; q < 4; ++q) dst[q] = make_uint4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
}

pgk_status dequant_nvf4_nk(const uint8_t* data, const uint8_t* scale, bf16* out, int n, int k, hipStream_t st) {
    PGK_REQUIRE(data && scale && out && n >= 1 && k >= 32 && k % 32 == 0, "dequant_nvf4_nk: bad arguments (n=%d k=%d)", n, k);
    const long long nblk = (long long)n * (k / 32);
    dequant_nvf4_nk_kernel<<<(unsigned)ceil_div(nblk, 256LL), 256, 0, st>>>(data, scale, out, nblk);
    PGK_CHECK_HIP(hipGetLastError());
    return PGK_OK;
}

// ---- weight-only GEMV (nvf4_kernels.cu:19-235) ------------------------------------------------------------------
// Workgroup = 256 threads = 8 column lanes (16 adjacent columns each: one dwordx4 per k-pair row, 128 columns = one
// 128-byte segment per row) x 32 k-lanes.  The workgroup owns scale blocks [sb0, sb1) of its 128 columns; k-lane kl
// takes blocks sb0 + kl, sb0 + kl + 32, ...: 16 row loads + 1 scale load per block, all issued before any is used.
// VEC = false is the byte-load form for a row stride (N) or base pointer that is not 16-byte aligned.
constexpr int NV_TN = 128, NV_KLANES = 32, NV_THREADS = 256, NV_MAX_BPW = 128;

template <bool VEC>
__device__ __forceinline__ uint4 nv_load16(const uint8_t* p, int col0, int N, bool ok) {
    if constexpr (VEC) {
        return ok ? *reinterpret_cast<const uint4*>(p + col0) : make_uint4(0, 0, 0, 0);
    } else {
        uint32_t w[4] = {0, 0, 0, 0};
        if (ok) {
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (col0 + j < N) w[j >> 2] |= (uint32_t)p[col0 + j] << (8 * (j & 3));
        }
        return make_uint4(w[0], w[1], w[2], w[3]);
    }
}

__device__ __forceinline__ uint32_t u4_word(const uint4& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }

// column B of a dword of 4 columns: byte B of dw is its (k, k+1) pair.  The conversion gives low nibble (k even)
// -> .x, high nibble (k odd) -> .y.  Its scale operand is used as a power of two only (the exponent of the f32,
// as an E8M0 MX scale), so it gets 1.0 and the block's scale byte is applied once per block by the caller.
template <int B>
__device__ __forceinline__ void nv_fma_byte(uint32_t dw, f32x2_n av, float& acc) {
    const f32x2_n b = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(dw, 1.0f, B);
    acc = fmaf(av.x, b.x, acc);
    acc = fmaf(av.y, b.y, acc);
}

template <bool VEC>
__global__ __launch_bounds__(NV_THREADS) void gemv_nvf4_kernel(const bf16* a, const uint8_t* data, const uint8_t* scale, bf16* c,
                                                               float* partial, int K, int N, float alpha, int bpw) {
    extern __shared__ __attribute__((aligned(16))) float nv_smem[];   // red [32][128] | a [bpw * 32]
    float* red = nv_smem;
    float* as = nv_smem + NV_KLANES * NV_TN;
    const int tid = threadIdx.x, cl = tid & 7, kl = tid >> 3;
    const int n0 = blockIdx.x * NV_TN, col0 = n0 + cl * 16;
    const int nsb = (K + 31) >> 5, KP = K >> 1;
    const int sb0 = blockIdx.y * bpw, sb1 = min(sb0 + bpw, nsb);
    const int k_lo = sb0 * 32;
    for (int i = tid; i < bpw * 32; i += NV_THREADS) as[i] = k_lo + i < K ? to_f(a[k_lo + i]) : 0.f;
    __syncthreads();

    const bool col_ok = col0 < N;
    float acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;
    for (int sb = sb0 + kl; sb < sb1; sb += NV_KLANES) {
        uint4 d[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = sb * 16 + r;
            d[r] = nv_load16<VEC>(data + (size_t)row * N, col0, N, col_ok && row < KP);
        }
        const uint4 sv = nv_load16<VEC>(scale + (size_t)sb * N, col0, N, col_ok);
        const float* ab = as + (sb - sb0) * 32;
        float blk[16];   // sum over the block of a[k] * e2m1, per column (exact products, fp32 sums)
#pragma unroll
        for (int j = 0; j < 16; ++j) blk[j] = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const f32x2_n av = *reinterpret_cast<const f32x2_n*>(ab + 2 * r);
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const uint32_t dw = u4_word(d[r], w);
                nv_fma_byte<0>(dw, av, blk[4 * w + 0]);
                nv_fma_byte<1>(dw, av, blk[4 * w + 1]);
                nv_fma_byte<2>(dw, av, blk[4 * w + 2]);
                nv_fma_byte<3>(dw, av, blk[4 * w + 3]);
            }
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = fmaf(blk[j], nvf4_scale_value((u4_word(sv, j >> 2) >> (8 * (j & 3))) & 0xFFu), acc[j]);
    }
#pragma unroll
    for (int j = 0; j < 16; j += 4)
        *reinterpret_cast<f32x4_t*>(red + kl * NV_TN + cl * 16 + j) = f32x4_t{acc[j], acc[j + 1], acc[j + 2], acc[j + 3]};
    __syncthreads();
    if (tid < NV_TN && n0 + tid < N) {
        float sum = 0.f;
        for (int i = 0; i < NV_KLANES; ++i) sum += red[i * NV_TN + tid];   // fixed order
        if (gridDim.y == 1) c[n0 + tid] = from_f<bf16>(alpha * sum);
        else partial[(size_t)blockIdx.y * N + n0 + tid] = sum;
    }
}

__global__ __launch_bounds__(256) void gemv_nvf4_reduce_kernel(const float* partial, bf16* c, int N, int S, float alpha) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float sum = 0.f;
    for (int s = 0; s < S; ++s) sum += partial[(size_t)s * N + n];   // fixed order
    c[n] = from_f<bf16>(alpha * sum);
}

// workgroups along K: enough workgroups for 256 CUs (>= 1024 when K allows), at most NV_MAX_BPW blocks (4096 k) each
static void gemv_nvf4_split(int K, int N, int* S, int* bpw) {
    const int nsb = (K + 31) / 32, tiles = ceil_div(N, NV_TN);
    int s = std::min(ceil_div(nsb, NV_KLANES), std::max(1, ceil_div(1024, tiles)));
    s = std::max(s, ceil_div(nsb, NV_MAX_BPW));
    *bpw = ceil_div(nsb, s);
    *S = ceil_div(nsb, *bpw);
}

// ---- unit-scale e2m1 packing for the GEMM (nvf4_cutlass.cu:157-317) ----------------------------------------------

// the reference's branchless bf16_to_nvf4_e2m1: NaN -> +0, +-inf and |x| >= 5 -> +-6, ties away from zero
__device__ __forceinline__ uint32_t e2m1_unit(float x) {
    const float a = fabsf(x);
    const uint32_t c = (uint32_t)(a >= 0.25f) + (uint32_t)(a >= 0.75f) + (uint32_t)(a >= 1.25f) + (uint32_t)(a >= 1.75f) +
                       (uint32_t)(a >= 2.5f) + (uint32_t)(a >= 3.5f) + (uint32_t)(a >= 5.0f);
    return (x < 0.f ? 8u : 0u) | c;
}

// out [rows, Kp/2]: row r holds k = 0..Kp-1 of operand row r (A [rows, K]) or column r (transpose: B [K, rows]),
// zero past K.  One thread per (row, 32 k) writes 16 bytes; consecutive threads walk k (A) or the row (B), so
// the bf16 reads are coalesced either way.
template <bool TRANS>
__global__ __launch_bounds__(256) void quantize_e2m1_kernel(const bf16* x, uint8_t* out, int rows, int K, int Kp) {
    const int G = Kp >> 5;
    const int t = blockIdx.x * 256 + threadIdx.x;   // rows * G < 2^31 (host check)
    if (t >= rows * G) return;
    const int r = TRANS ? t % rows : t / G;
    const int g = TRANS ? t / rows : t % G;
    uint32_t w[4] = {0, 0, 0, 0};
    if (g * 32 < K) {   // K % 32 == 0: a group is all in or all out
        float v[32];
        if constexpr (TRANS) {
#pragma unroll
            for (int i = 0; i < 32; ++i) v[i] = to_f(x[(size_t)(g * 32 + i) * rows + r]);
        } else {
#pragma unroll
            for (int i = 0; i < 32; i += 8) {
                Vec<bf16> vv;
                float f[8];
                vv.load(x + (size_t)r * K + g * 32 + i);
                vv.to_float(f);
#pragma unroll
                for (int j = 0; j < 8; ++j) v[i + j] = f[j];
            }
        }
#pragma unroll
        for (int i = 0; i < 32; ++i) w[i >> 3] |= e2m1_unit(v[i]) << (4 * (i & 7));
    }
    *reinterpret_cast<uint4*>(out + (size_t)r * (Kp >> 1) + g * 16) = make_uint4(w[0], w[1], w[2], w[3]);
}

// ---- FP4 NT GEMM ---------------------------------------------------------------------------------------------
// D[m][n] = sum_k e2m1(A[m][k]) * e2m1(B[n][k]), A / B packed [rows, Kp/2].  128 x 128 tiles, 4 waves of 64 x 64,
// 256 k (128 bytes per row) per step staged through registers into a double-buffered swizzled LDS tile (the
// structure of ops_fp8_gemm.hip).  One step is two MFMAs per 16 x 16 output tile: bytes 0..63 then 64..127 of each
// row; lane l supplies the 16 bytes 16*(l>>4) .. +15 of row l & 15 of each half to both operands.  A and B use the
// same (lane, byte, nibble) -> k assignment, so the contraction pairs matching k in whatever order the hardware
// walks the nibbles, and every product (a multiple of 1/4, at most 36) and sum is exact in fp32.
constexpr int F4_BM = 128, F4_BN = 128, F4_THREADS = 256;
constexpr int F4_TILE = 128 * 128;   // bytes of one staged operand tile: 128 rows x 128 bytes (256 k)

__global__ __launch_bounds__(F4_THREADS) void gemm_fp4_kernel(const uint8_t* A, const uint8_t* B, bf16* D, int M, int N, int Kp) {
    extern __shared__ __attribute__((aligned(16))) char f4_smem[];   // A[2] | B[2]
    auto As = [&](int buf) -> char* { return f4_smem + buf * F4_TILE; };
    auto Bs = [&](int buf) -> char* { return f4_smem + 2 * F4_TILE + buf * F4_TILE; };

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1, q = lane >> 4;
    const int m0 = blockIdx.y * F4_BM, n0 = blockIdx.x * F4_BN;
    const int RB = Kp >> 1;                 // bytes per packed row
    const int KT = (RB + 127) >> 7;         // steps; the last one is half empty when Kp % 256 == 128

    uint4 ra0, ra1, ra2, ra3, rb0, rb1, rb2, rb3;   // named scalars: a staging array would land in scratch
    const int srow = tid >> 3, skc = tid & 7;
    const uint8_t* a_p0 = A + (size_t)min(m0 + srow, M - 1) * RB + skc * 16;
    const uint8_t* a_p1 = A + (size_t)min(m0 + 32 + srow, M - 1) * RB + skc * 16;
    const uint8_t* a_p2 = A + (size_t)min(m0 + 64 + srow, M - 1) * RB + skc * 16;
    const uint8_t* a_p3 = A + (size_t)min(m0 + 96 + srow, M - 1) * RB + skc * 16;
    const uint8_t* b_p0 = B + (size_t)min(n0 + srow, N - 1) * RB + skc * 16;
    const uint8_t* b_p1 = B + (size_t)min(n0 + 32 + srow, N - 1) * RB + skc * 16;
    const uint8_t* b_p2 = B + (size_t)min(n0 + 64 + srow, N - 1) * RB + skc * 16;
    const uint8_t* b_p3 = B + (size_t)min(n0 + 96 + srow, N - 1) * RB + skc * 16;
    const int st_off = swz128_off(srow, skc);
    auto load_tiles = [&](int kt) {
        // past the packed row (the second half of the last step when Kp % 256 == 128): load chunk 0 again and
        // zero it.  A select, not a branch: a branch here makes hipcc keep the staging registers in scratch.
        const bool ok = kt * 128 + skc * 16 < RB;
        const int kb = ok ? kt * 128 : -skc * 16;
        auto ld = [&](const uint8_t* p) {
            const uint4 v = *reinterpret_cast<const uint4*>(p + kb);
            return make_uint4(ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u);
        };
        ra0 = ld(a_p0); ra1 = ld(a_p1); ra2 = ld(a_p2); ra3 = ld(a_p3);
        rb0 = ld(b_p0); rb1 = ld(b_p1); rb2 = ld(b_p2); rb3 = ld(b_p3);
    };
    auto store_tiles = [&](int buf) {
        char* a = As(buf) + st_off;
        char* b = Bs(buf) + st_off;
        *reinterpret_cast<uint4*>(a) = ra0; *reinterpret_cast<uint4*>(a + 32 * 128) = ra1;
        *reinterpret_cast<uint4*>(a + 64 * 128) = ra2; *reinterpret_cast<uint4*>(a + 96 * 128) = ra3;
        *reinterpret_cast<uint4*>(b) = rb0; *reinterpret_cast<uint4*>(b + 32 * 128) = rb1;
        *reinterpret_cast<uint4*>(b + 64 * 128) = rb2; *reinterpret_cast<uint4*>(b + 96 * 128) = rb3;
    };

    f32x4_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    load_tiles(0);
    store_tiles(0);
    __syncthreads();
    for (int kt = 0; kt < KT; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < KT) load_tiles(kt + 1);
#pragma unroll
        for (int h = 0; h < 2; ++h) {   // the two 128-k halves of the step
            i32x8_t fa[4], fb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int ar = wm * 64 + i * 16 + (lane & 15), br = wn * 64 + i * 16 + (lane & 15);
                const uint4 a0 = *reinterpret_cast<const uint4*>(As(buf) + swz128_off(ar, 4 * h + q));
                const uint4 b0 = *reinterpret_cast<const uint4*>(Bs(buf) + swz128_off(br, 4 * h + q));
                // e2m1 operands occupy the low 4 registers of the 8-register operand
                fa[i] = i32x8_t{(int)a0.x, (int)a0.y, (int)a0.z, (int)a0.w, 0, 0, 0, 0};
                fb[i] = i32x8_t{(int)b0.x, (int)b0.y, (int)b0.z, (int)b0.w, 0, 0, 0, 0};
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fa[i], fb[j], acc[i][j], 4, 4, 0, 127, 0, 127);
        }
        if (kt + 1 < KT) store_tiles(buf ^ 1);
        __syncthreads();
    }

    // C/D map of the 16x16 MFMA shapes: col = lane & 15, row = (lane >> 4) * 4 + reg
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = n0 + wn * 64 + j * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wm * 64 + i * 16 + q * 4 + r;
                if (row < M && col < N) D[(size_t)row * N + col] = from_f<bf16>(acc[i][j][r]);
            }
        }
}

static int nvf4_kp(int k) { return (k + 127) / 128 * 128; }

}  // namespace pgk

using namespace pgk;

extern "C" {

pgk_status pgk_quantize_nvf4(const void* x_kn, uint8_t* data, uint8_t* scale, int k, int n, pgk_stream s) {
    PGK_REQUIRE(x_kn && data && scale, "pgk_quantize_nvf4: null argument");
    PGK_REQUIRE(k >= 2 && k % 2 == 0 && n >= 1, "pgk_quantize_nvf4: k=%d must be positive and even (n=%d)", k, n);
    quantize_nvf4_kernel<<<dim3(ceil_div(n, 256), ceil_div(k, 32)), 256, 0, resolve_stream(s)>>>((const bf16*)x_kn, data, scale, k, n);
    PGK_CHECK_HIP(hipGetLastError());
    return PGK_OK;
}

pgk_status pgk_quantize_nvf4_nk(const void* x_nk, uint8_t* data, uint8_t* scale, int n, int k, pgk_stream s) {
    PGK_REQUIRE(x_nk && data && scale, "pgk_quantize_nvf4_nk: null argument");
    PGK_REQUIRE(n >= 1 && k >= 32 && k % 32 == 0, "pgk_quantize_nvf4_nk: k=%d must be a positive multiple of 32 (n=%d)", k, n);
    PGK_REQUIRE(((uintptr_t)x_nk & 15) == 0 && ((uintptr_t)data & 15) == 0, "pgk_quantize_nvf4_nk: input and data must be 16-byte aligned");
    const long long nblk = (long long)n * (k / 32);
    quantize_nvf4_nk_kernel<<<(unsigned)ceil_div(nblk, 256LL), 256, 0, resolve_stream(s)>>>((const bf16*)x_nk, data, scale, nblk);
    PGK_CHECK_HIP(hipGetLastError());
    return PGK_OK;
}

size_t pgk_gemv_nvf4_workspace_bytes(int k, int n) {
    if (k < 2 || n < 1) return 0;
    int S, bpw;
    gemv_nvf4_split(k, n, &S, &bpw);
    return S > 1 ? (size_t)S * n * sizeof(float) : 0;
}

pgk_status pgk_gemv_nvf4_bf16(const void* a, const uint8_t* data, const uint8_t* scale, void* c, void* workspace, int k, int n,
                              float alpha, pgk_stream s) {
    PGK_REQUIRE(a && data && scale && c, "pgk_gemv_nvf4_bf16: null argument");
    PGK_REQUIRE(k >= 2 && k % 2 == 0 && n >= 1, "pgk_gemv_nvf4_bf16: k=%d must be positive and even (n=%d)", k, n);
    int S, bpw;
    gemv_nvf4_split(k, n, &S, &bpw);
    PGK_REQUIRE(S == 1 || workspace, "pgk_gemv_nvf4_bf16: k=%d n=%d needs a workspace of pgk_gemv_nvf4_workspace_bytes", k, n);
    hipStream_t st = resolve_stream(s);
    const bool vec = n % 16 == 0 && ((uintptr_t)data & 15) == 0 && ((uintptr_t)scale & 15) == 0;
    const dim3 grid(ceil_div(n, NV_TN), S);
    const size_t lds = ((size_t)NV_KLANES * NV_TN + (size_t)bpw * 32) * sizeof(float);
    if (vec) gemv_nvf4_kernel<true><<<grid, NV_THREADS, lds, st>>>((const bf16*)a, data, scale, (bf16*)c, (float*)workspace, k, n, alpha, bpw);
    else gemv_nvf4_kernel<false><<<grid, NV_THREADS, lds, st>>>((const bf16*)a, data, scale, (bf16*)c, (float*)workspace, k, n, alpha, bpw);
    PGK_CHECK_HIP(hipGetLastError());
    if (S > 1) {
        gemv_nvf4_reduce_kernel<<<ceil_div(n, 256), 256, 0, st>>>((const float*)workspace, (bf16*)c, n, S, alpha);
        PGK_CHECK_HIP(hipGetLastError());
    }
    return PGK_OK;
}

pgk_status pgk_quantize_e2m1_unit(const void* x, uint8_t* out, int rows, int k, int transpose, pgk_stream s) {
    PGK_REQUIRE(x && out, "pgk_quantize_e2m1_unit: null argument");
    PGK_REQUIRE(rows >= 1 && k >= 32 && k % 32 == 0, "pgk_quantize_e2m1_unit: k=%d must be a positive multiple of 32 (rows=%d)", k, rows);
    PGK_REQUIRE(((uintptr_t)out & 15) == 0 && (transpose || ((uintptr_t)x & 15) == 0), "pgk_quantize_e2m1_unit: misaligned buffer");
    const int kp = nvf4_kp(k);
    PGK_REQUIRE((long long)rows * (kp / 32) < (1LL << 31) - 256, "pgk_quantize_e2m1_unit: rows=%d k=%d too large", rows, k);
    const unsigned grid = (unsigned)ceil_div((long long)rows * (kp / 32), 256);
    hipStream_t st = resolve_stream(s);
    if (transpose) quantize_e2m1_kernel<true><<<grid, 256, 0, st>>>((const bf16*)x, out, rows, k, kp);
    else quantize_e2m1_kernel<false><<<grid, 256, 0, st>>>((const bf16*)x, out, rows, k, kp);
    PGK_CHECK_HIP(hipGetLastError());
    return PGK_OK;
}

pgk_status pgk_gemm_fp4_nt(const uint8_t* a_packed, const uint8_t* b_packed, void* d, int m, int n, int kp, pgk_stream s) {
    PGK_REQUIRE(a_packed && b_packed && d, "pgk_gemm_fp4_nt: null argument");
    PGK_REQUIRE(m >= 1 && n >= 1 && kp >= 128 && kp % 128 == 0, "pgk_gemm_fp4_nt: kp=%d must be a positive multiple of 128 (m=%d n=%d)",
                kp, m, n);
    PGK_REQUIRE(((uintptr_t)a_packed & 15) == 0 && ((uintptr_t)b_packed & 15) == 0, "pgk_gemm_fp4_nt: misaligned operand");
    constexpr size_t LDS = 4 * (size_t)F4_TILE;
    static bool attr_done = false;
    if (!attr_done) {
        PGK_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_fp4_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS));
        attr_done = true;
    }
    gemm_fp4_kernel<<<dim3(ceil_div(n, F4_BN), ceil_div(m, F4_BM)), F4_THREADS, LDS, resolve_stream(s)>>>(a_packed, b_packed, (bf16*)d, m, n, kp);
    PGK_CHECK_HIP(hipGetLastError());
    return PGK_OK;
}

size_t pgk_gemm_nvf4_workspace_bytes(int m, int n, int k) {
    if (m < 1 || n < 1 || k < 1) return 0;
    return ((size_t)m + n) * (size_t)(nvf4_kp(k) / 2);
}

}  // extern "C"
