// Integer matmuls and the int8 quantiser (reference: native/bindings/gemm/int.cpp, native/ops/matmul/gemv/int4_int4/sm120,
// native/bindings/quantize.cpp + native/ops/quantize/quantize_kernels.cuh).
//
//   pgk_gemm_int8_nt          D[M,N] int32 = A[M,K] int8 . B[N,K]^T int8.  Exact: every product and partial sum is an integer
//                             in int32; the result is the true sum wherever that fits int32 and its two's-complement wrap
//                             (the sum mod 2^32) where it does not.
//   pgk_gemm_int8_dequant_nt  the same accumulator, stored as out = (float)acc * a_scale[m] * w_scale[n] (+ bias[n]).
//   pgk_gemm_int4_nt          A [M,K/2], B [N,K/2] packed signed nibbles (k even low, k + 1 high), exact int32 accumulator,
//                             D = saturate(roundf((float)acc * scale_a * scale_b * descale_d)) as int32 or int8; with all three
//                             factors 1.0f the int32 output is the accumulator itself.
//   pgk_gemv_int4             C[N] int32 = saturate(roundf((float)(sum_k a[k] B[n][k]) * scale_a * scale_b)).
//   pgk_quantize_int8_rows / pgk_dequantize_int8_rows / pgk_linear_int8: per-row symmetric int8 and the weight-only linear.
//
// Tile kernel (gemm_int_tile_kernel): 256 threads = 2 x 2 waves, BM x 128 block tile (BM = 128 or 64, int8_plan.h), K tiles of
// 128 BYTES per LDS row in the XOR swizzle of mfma_common.hip.h, staged global -> VGPR -> LDS in 16-byte chunks with two LDS
// buffers: the global loads of tile t + 1 are issued before the MFMAs of tile t and written to LDS after them.  One
// v_mfma_i32_16x16x64_i8 consumes a 16-byte fragment (ds_read_b128) of 16 rows of each operand, so a 128-byte row is two MFMAs
// per 16 x 16 output tile.  Lane l supplies bytes 16 * (l >> 4) .. + 15 of row l & 15 of each 64-byte half to BOTH operands:
// the contraction pairs matching k in whatever order the hardware walks the bytes.
// Packed int4 runs on the same walk with the packed bytes staged as they are (a 128-byte LDS row = 256 k).  For a packed word w,
// (w << 4) & 0xF0F0F0F0 and w & 0xF0F0F0F0 are its low and high nibble planes as int8 values 16 x: two MFMAs per fragment
// (low . low, high . high) accumulate 256 x the sum and the epilogue shifts right by 8, which is exact.  That form needs
// K * 2^14 < 2^31 (int8_plan.h); beyond it the planes are sign-extended to the nibble values themselves.
// Rows past M / N and bytes past the row are zero in LDS; no load leaves the operands.

#include "gemm_tile_core.hip.h"
#include "gemv_core.hip.h"
#include "int8_plan.h"
#include "mfma_common.hip.h"
#include "pgk_internal.h"

#include <climits>
#include <string>

namespace pgk {

typedef int i32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

enum IntEpi { EPI_I32 = 0, EPI_DEQUANT = 1, EPI_SCALED = 2 };
enum IntMode { IM_I8 = 0, IM_I4_PLANES = 1, IM_I4_EXT = 2 };

struct IntEpiArgs {
    const float* a_scale;   // EPI_DEQUANT: [M]
    const float* w_scale;   //              [N]
    const void* bias;       //              [N] in the output dtype, or NULL
    float sa, sb, dd;       // EPI_SCALED
};

template <class OT> __device__ __forceinline__ OT saturate_to(float r);
template <> __device__ __forceinline__ int32_t saturate_to<int32_t>(float r) {
    if (!(r == r)) return 0;
    return r >= 2147483648.f ? INT_MAX : r <= -2147483648.f ? INT_MIN : (int32_t)r;
}
template <> __device__ __forceinline__ int8_t saturate_to<int8_t>(float r) {
    if (!(r == r)) return 0;
    return (int8_t)(int)fminf(fmaxf(r, -128.f), 127.f);
}

// One output element.  The products are fp32, left to right, never contracted with the bias add; one rounding to OT.
template <int EPI, class OT>
__device__ __forceinline__ void int_epilogue(int acc, OT* D, int row, int col, int N, const IntEpiArgs& e) {
#pragma clang fp contract(off)
    const size_t at = (size_t)row * N + col;
    if constexpr (EPI == EPI_I32) {
        D[at] = acc;
    } else if constexpr (EPI == EPI_DEQUANT) {
        float r = (float)acc * e.a_scale[row] * e.w_scale[col];
        if (e.bias) r = r + to_f(static_cast<const OT*>(e.bias)[col]);
        D[at] = from_f<OT>(r);
    } else {
        const float r = (float)acc * e.sa * e.sb * e.dd;
        D[at] = saturate_to<OT>(roundf(r));
    }
}

// the 8 nibbles of the low / high plane of 4 packed words, sign-extended to int8 (IM_I4_EXT): per byte (x ^ 8) - 8 without a
// borrow between bytes
__device__ __forceinline__ u32x4_t sext_nibbles(u32x4_t x) {   // x: nibbles in the low half of every byte
    const u32x4_t y = x ^ 0x08080808u;
    return ((y | 0x80808080u) - 0x08080808u) ^ 0x80808080u;
}

__device__ __forceinline__ i32x4_t mfma_i8(u32x4_t a, u32x4_t b, i32x4_t c) {
    return __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4_t, a), __builtin_bit_cast(i32x4_t, b), c, 0, 0, 0);
}

constexpr int IG_BN = 128, IG_THREADS = 256;
constexpr size_t int_tile_lds_bytes(int bm) { return 2 * (size_t)(bm + IG_BN) * 128; }

// RB: bytes per operand row (K for int8, K / 2 for packed int4), a multiple of 16.
template <int BM, int MODE, int EPI, class OT>
__global__ __launch_bounds__(IG_THREADS) void gemm_int_tile_kernel(const uint8_t* A, const uint8_t* B, OT* D, int M, int N, int RB,
                                                                  int ntn, IntEpiArgs e) {
    constexpr int WM = BM / 2, TM = WM / 16, TN = 4;
    constexpr int A_TILE = BM * 128, B_TILE = IG_BN * 128;
    extern __shared__ __attribute__((aligned(16))) char ig_smem[];   // A[2] | B[2]
    auto As = [&](int buf) -> char* { return ig_smem + buf * A_TILE; };
    auto Bs = [&](int buf) -> char* { return ig_smem + 2 * A_TILE + buf * B_TILE; };

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1, q = lane >> 4;
    const int m0 = (int)(blockIdx.x / ntn) * BM, n0 = (int)(blockIdx.x % ntn) * IG_BN;
    const int KT = (RB + 127) >> 7;

    // staging registers: named scalars, not arrays (at this register pressure hipcc leaves a staging ARRAY in scratch)
    uint4 ra0, ra1, ra2, ra3, rb0, rb1, rb2, rb3;
    const int srow = tid >> 3, skc = tid & 7;
    auto row_ptr = [&](const uint8_t* base, int r, int nrows) { return base + (size_t)min(r, nrows - 1) * RB + skc * 16; };
    const uint8_t* a_p0 = row_ptr(A, m0 + srow, M);
    const uint8_t* a_p1 = row_ptr(A, m0 + 32 + srow, M);
    const uint8_t* a_p2 = row_ptr(A, m0 + 64 + srow, M);
    const uint8_t* a_p3 = row_ptr(A, m0 + 96 + srow, M);
    const uint8_t* b_p0 = row_ptr(B, n0 + srow, N);
    const uint8_t* b_p1 = row_ptr(B, n0 + 32 + srow, N);
    const uint8_t* b_p2 = row_ptr(B, n0 + 64 + srow, N);
    const uint8_t* b_p3 = row_ptr(B, n0 + 96 + srow, N);
    const bool a_ok0 = m0 + srow < M, a_ok1 = m0 + 32 + srow < M, a_ok2 = m0 + 64 + srow < M, a_ok3 = m0 + 96 + srow < M;
    const bool b_ok0 = n0 + srow < N, b_ok1 = n0 + 32 + srow < N, b_ok2 = n0 + 64 + srow < N, b_ok3 = n0 + 96 + srow < N;
    const int st_off = swz128_off(srow, skc);   // rows srow + 32 i share the swizzle (32 % 8 == 0)
    auto load_tiles = [&](int kt) {
        // a chunk past the row (K tail) or of a row past M / N: load chunk 0 of a real row and zero it.  A select, not a
        // branch: a branch here makes hipcc keep the staging registers in scratch.
        const bool kok = kt * 128 + skc * 16 < RB;
        const int kb = kok ? kt * 128 : -skc * 16;
        auto ld = [&](const uint8_t* p, bool rok) {
            const uint4 v = *reinterpret_cast<const uint4*>(p + kb);
            const bool ok = kok && rok;
            return make_uint4(ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u);
        };
        ra0 = ld(a_p0, a_ok0); ra1 = ld(a_p1, a_ok1);
        if constexpr (BM == 128) { ra2 = ld(a_p2, a_ok2); ra3 = ld(a_p3, a_ok3); }
        rb0 = ld(b_p0, b_ok0); rb1 = ld(b_p1, b_ok1); rb2 = ld(b_p2, b_ok2); rb3 = ld(b_p3, b_ok3);
    };
    auto store_tiles = [&](int buf) {
        char* a = As(buf) + st_off;
        char* b = Bs(buf) + st_off;
        *reinterpret_cast<uint4*>(a) = ra0; *reinterpret_cast<uint4*>(a + 32 * 128) = ra1;
        if constexpr (BM == 128) { *reinterpret_cast<uint4*>(a + 64 * 128) = ra2; *reinterpret_cast<uint4*>(a + 96 * 128) = ra3; }
        *reinterpret_cast<uint4*>(b) = rb0; *reinterpret_cast<uint4*>(b + 32 * 128) = rb1;
        *reinterpret_cast<uint4*>(b + 64 * 128) = rb2; *reinterpret_cast<uint4*>(b + 96 * 128) = rb3;
    };

    i32x4_t acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = i32x4_t{0, 0, 0, 0};

    load_tiles(0);
    store_tiles(0);
    __syncthreads();
    for (int kt = 0; kt < KT; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < KT) load_tiles(kt + 1);
#pragma unroll
        for (int h = 0; h < 2; ++h) {   // the two 64-byte halves of the row
            u32x4_t fa[TM], fb[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i)
                fa[i] = *reinterpret_cast<const u32x4_t*>(As(buf) + swz128_off(wm * WM + i * 16 + (lane & 15), 4 * h + q));
#pragma unroll
            for (int j = 0; j < TN; ++j)
                fb[j] = *reinterpret_cast<const u32x4_t*>(Bs(buf) + swz128_off(wn * 64 + j * 16 + (lane & 15), 4 * h + q));
            if constexpr (MODE == IM_I8) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) acc[i][j] = mfma_i8(fa[i], fb[j], acc[i][j]);
            } else {
                u32x4_t al[TM], ah[TM], bl[TN], bh[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    if constexpr (MODE == IM_I4_PLANES) { al[i] = (fa[i] << 4) & 0xF0F0F0F0u; ah[i] = fa[i] & 0xF0F0F0F0u; }
                    else { al[i] = sext_nibbles(fa[i] & 0x0F0F0F0Fu); ah[i] = sext_nibbles((fa[i] >> 4) & 0x0F0F0F0Fu); }
                }
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    if constexpr (MODE == IM_I4_PLANES) { bl[j] = (fb[j] << 4) & 0xF0F0F0F0u; bh[j] = fb[j] & 0xF0F0F0F0u; }
                    else { bl[j] = sext_nibbles(fb[j] & 0x0F0F0F0Fu); bh[j] = sext_nibbles((fb[j] >> 4) & 0x0F0F0F0Fu); }
                }
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        acc[i][j] = mfma_i8(al[i], bl[j], acc[i][j]);
                        acc[i][j] = mfma_i8(ah[i], bh[j], acc[i][j]);
                    }
            }
        }
        if (kt + 1 < KT) store_tiles(buf ^ 1);
        __syncthreads();
    }

    // C/D map of the 16x16 MFMA shapes: col = lane & 15, row = (lane >> 4) * 4 + reg
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int col = n0 + wn * 64 + j * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wm * WM + i * 16 + q * 4 + r;
                const int v = MODE == IM_I4_PLANES ? acc[i][j][r] >> 8 : acc[i][j][r];   // 256 x the sum: the shift is exact
                if (row < M && col < N) int_epilogue<EPI, OT>(v, D, row, col, N, e);
            }
        }
}

// ---- correctness kernel: any K, any alignment; one output per thread on v_dot4_i32_i8 / v_dot8_i32_i4 over words gathered byte
// by byte, scalar tail.  The same exact accumulator and the same epilogue as the tile kernel. ---------------------------------
__device__ __forceinline__ int word_at(const uint8_t* p) { return (int)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24)); }
__device__ __forceinline__ int nib_lo(uint8_t b) { return (int)(int8_t)(b << 4) >> 4; }
__device__ __forceinline__ int nib_hi(uint8_t b) { return (int)(int8_t)b >> 4; }

template <bool I4, int EPI, class OT>
__global__ __launch_bounds__(256) void gemm_int_simple_kernel(const uint8_t* A, const uint8_t* B, OT* D, int M, int N, int RB, int ntn,
                                                             IntEpiArgs e) {
    const int col = (int)(blockIdx.x % ntn) * 16 + (threadIdx.x & 15), row = (int)(blockIdx.x / ntn) * 16 + (threadIdx.x >> 4);
    if (row >= M || col >= N) return;
    const uint8_t* a = A + (size_t)row * RB;
    const uint8_t* b = B + (size_t)col * RB;
    int acc = 0, i = 0;
    for (; i + 4 <= RB; i += 4) {
        if constexpr (I4) acc = __builtin_amdgcn_sdot8(word_at(a + i), word_at(b + i), acc, false);
        else acc = __builtin_amdgcn_sdot4(word_at(a + i), word_at(b + i), acc, false);
    }
    for (; i < RB; ++i) {
        if constexpr (I4) acc += nib_lo(a[i]) * nib_lo(b[i]) + nib_hi(a[i]) * nib_hi(b[i]);
        else acc += (int)(int8_t)a[i] * (int)(int8_t)b[i];
    }
    int_epilogue<EPI, OT>(acc, D, row, col, N, e);
}

template <int MODE, int EPI, class OT>
static pgk_status launch_int_gemm(IntGemmKernel kern, const void* A, const void* B, OT* D, int M, int N, int RB, const IntEpiArgs& e,
                                  hipStream_t st) {
    const uint8_t* a = static_cast<const uint8_t*>(A);
    const uint8_t* b = static_cast<const uint8_t*>(B);
    if (kern == IG_SIMPLE) {
        const int ntn = ceil_div(N, 16);
        PGK_REQUIRE((long long)ntn * ceil_div(M, 16) < (1LL << 31), "int gemm: M=%d N=%d too large", M, N);
        gemm_int_simple_kernel<MODE != IM_I8, EPI, OT><<<(unsigned)(ntn * ceil_div(M, 16)), 256, 0, st>>>(a, b, D, M, N, RB, ntn, e);
        PGK_LAUNCH_CHECK();
        return PGK_OK;
    }
    const int ntn = ceil_div(N, IG_BN);
    if (kern == IG_TILE128)
        return launch_dyn_lds<gemm_int_tile_kernel<128, MODE, EPI, OT>>(dim3((unsigned)(ntn * ceil_div(M, 128))), IG_THREADS, int_tile_lds_bytes(128),
                                                                       true, st, a, b, D, M, N, RB, ntn, e);
    return launch_dyn_lds<gemm_int_tile_kernel<64, MODE, EPI, OT>>(dim3((unsigned)(ntn * ceil_div(M, 64))), IG_THREADS, int_tile_lds_bytes(64),
                                                                  true, st, a, b, D, M, N, RB, ntn, e);
}

// ---- int4 GEMV ---------------------------------------------------------------------------------------------------------------
// A wave owns R consecutive rows of B and streams them once: lane l takes the 16-byte chunks l, l + 64, ... of every row (32
// nibbles per load, non-temporal) and the matching 16 bytes of a, which stay in registers for all R rows.  v_dot8_i32_i4 takes
// the packed words as they are (nibble i of one word meets nibble i of the other).  The 64 partial sums meet in a DPP tree.
template <int CTRL> __device__ __forceinline__ int dpp_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true); }
__device__ __forceinline__ int wave_sum_i32(int v) {
    v += dpp_i<DPP_XOR1>(v); v += dpp_i<DPP_XOR2>(v); v += dpp_i<DPP_HALF_MIRROR>(v); v += dpp_i<DPP_MIRROR>(v);
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48);
}
__device__ __forceinline__ int32_t gemv_int4_out(int acc, float sa, float sb) {
#pragma clang fp contract(off)
    return saturate_to<int32_t>(roundf((float)acc * sa * sb));
}

template <int R>
__global__ __launch_bounds__(256) void gemv_int4_kernel(const uint8_t* a, const uint8_t* B, int32_t* C, int N, int RB, float sa, float sb) {
    const int lane = threadIdx.x & 63;
    const int n0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * R;
    if (n0 >= N) return;   // the whole wave
    const uint8_t* rows[R];
#pragma unroll
    for (int r = 0; r < R; ++r) rows[r] = B + (size_t)min(n0 + r, N - 1) * RB;
    int acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0;
    const int nch = RB >> 4;
    for (int c = lane; c < nch; c += 64) {
        uint4 w[R];
#pragma unroll
        for (int r = 0; r < R; ++r) w[r] = load_nt16(rows[r] + (size_t)c * 16);
        const uint4 av = *reinterpret_cast<const uint4*>(a + (size_t)c * 16);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            acc[r] = __builtin_amdgcn_sdot8((int)av.x, (int)w[r].x, acc[r], false);
            acc[r] = __builtin_amdgcn_sdot8((int)av.y, (int)w[r].y, acc[r], false);
            acc[r] = __builtin_amdgcn_sdot8((int)av.z, (int)w[r].z, acc[r], false);
            acc[r] = __builtin_amdgcn_sdot8((int)av.w, (int)w[r].w, acc[r], false);
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int s = wave_sum_i32(acc[r]);
        if (lane == 0 && n0 + r < N) C[n0 + r] = gemv_int4_out(s, sa, sb);
    }
}

// any even K, any alignment: a wave per row, a byte per lane and step
__global__ __launch_bounds__(256) void gemv_int4_simple_kernel(const uint8_t* a, const uint8_t* B, int32_t* C, int N, int RB, float sa, float sb) {
    const int lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const uint8_t* row = B + (size_t)n * RB;
    int acc = 0;
    for (int i = lane; i < RB; i += 64) acc += nib_lo(a[i]) * nib_lo(row[i]) + nib_hi(a[i]) * nib_hi(row[i]);
    acc = wave_sum_i32(acc);
    if (lane == 0) C[n] = gemv_int4_out(acc, sa, sb);
}

// ---- quantiser / dequantiser ---------------------------------------------------------------------------------------------------
// q = clamp(rint(x / s), -128, 127) with the IEEE division and round-to-nearest-even of the reference's __float2int_rn(val /
// row_scale) (NaN -> 0 as there); s = max|x| / 127 floored at 1e-10, kept in fp32 for the quotient and stored in T.
__device__ __forceinline__ int8_t quant_int8(float x, float s) {
    const float t = rintf(x / s);
    return t == t ? (int8_t)(int)fminf(fmaxf(t, -128.f), 127.f) : (int8_t)0;
}

// A 256-thread workgroup per row.  CACHED: the row (<= 4096 elements) is read once and held in registers, 16 per thread.
constexpr int Q8_THREADS = 256, Q8_PER_THREAD = 16, Q8_CACHED_COLS = Q8_THREADS * Q8_PER_THREAD;
template <class T, bool CACHED>
__global__ __launch_bounds__(Q8_THREADS) void quantize_int8_rows_kernel(const T* x, int8_t* q, T* scale, int cols) {
    __shared__ float red[Q8_THREADS / 64];
    const T* xr = x + (size_t)blockIdx.x * cols;
    int8_t* qr = q + (size_t)blockIdx.x * cols;
    const int tid = threadIdx.x;
    float v[Q8_PER_THREAD];
    float amax = 0.f;
    if constexpr (CACHED) {
#pragma unroll
        for (int j = 0; j < Q8_PER_THREAD; ++j) {
            const int c = tid + j * Q8_THREADS;
            v[j] = c < cols ? to_f(xr[c]) : 0.f;
            amax = fmaxf(amax, fabsf(v[j]));   // fmaxf drops NaN
        }
    } else {
        for (int c = tid; c < cols; c += Q8_THREADS) amax = fmaxf(amax, fabsf(to_f(xr[c])));
    }
    amax = wave_max(amax);
    if ((tid & 63) == 0) red[tid >> 6] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float s = amax / 127.0f;
    if (s < 1e-10f) s = 1e-10f;
    if constexpr (CACHED) {
#pragma unroll
        for (int j = 0; j < Q8_PER_THREAD; ++j) {
            const int c = tid + j * Q8_THREADS;
            if (c < cols) qr[c] = quant_int8(v[j], s);
        }
    } else {
        for (int c = tid; c < cols; c += Q8_THREADS) qr[c] = quant_int8(to_f(xr[c]), s);
    }
    if (tid == 0) scale[blockIdx.x] = from_f<T>(s);
}

template <class T>
__global__ __launch_bounds__(256) void dequantize_int8_rows_kernel(const int8_t* q, const T* scale, T* out, size_t total, int cols) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < total) out[i] = from_f<T>((float)q[i] * to_f(scale[i / cols]));
}

// ---- weight-only linear: out[m][n] = (sum_k act[m][k] * W[n][k]) * scale[n] (+ bias[n]) -----------------------------------------
// The scale is per output channel, so it leaves the sum: the int8 weights enter the products as the integers they are (exact in
// fp32 and in both 16-bit types) and scale[n] / bias[n] are applied once per output.

// 16 int8 -> 16 floats
__device__ __forceinline__ void i8x16_to_f32(const uint4& w, float (&f)[16]) {
    const uint32_t d[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int j = 0; j < 16; ++j) f[j] = (float)(int)(int8_t)(d[j >> 2] >> (8 * (j & 3)));
}

// Few rows (M <= 8): a workgroup of 4 waves streams 16 weight rows once, 4 per wave; lane l takes the 16-byte chunks l, l + 64,
// ... of the current K chunk.  The activations of the chunk (L8_KC k of every row) sit in LDS in their 16-bit form.
constexpr int L8_RW = 4, L8_ROWS = 4 * L8_RW, L8_KC = 2048;
template <class T, int MT>
__global__ __launch_bounds__(256) void linear_int8_stream_kernel(const T* act, const int8_t* W, const T* scale, const T* bias, T* out, int M,
                                                                int N, int K) {
    __shared__ uint4 xs[MT * (L8_KC / 8)];   // [MT][L8_KC] of T
    const int tid = threadIdx.x, lane = tid & 63;
    const int n0 = blockIdx.x * L8_ROWS + (tid >> 6) * L8_RW;
    const int8_t* wrow[L8_RW];
#pragma unroll
    for (int r = 0; r < L8_RW; ++r) wrow[r] = W + (size_t)min(n0 + r, N - 1) * K;
    float acc[L8_RW][MT];
#pragma unroll
    for (int r = 0; r < L8_RW; ++r)
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[r][m] = 0.f;

    for (int k0 = 0; k0 < K; k0 += L8_KC) {
        const int kc = min(L8_KC, K - k0), c8 = kc >> 3;   // K % 16 == 0
        if (k0) __syncthreads();   // the previous chunk has been consumed
        for (int i = tid; i < MT * c8; i += 256) {
            const int m = i / c8, c = i - m * c8;
            xs[m * (L8_KC / 8) + c] = m < M ? *reinterpret_cast<const uint4*>(act + (size_t)m * K + k0 + c * 8) : make_uint4(0, 0, 0, 0);
        }
        __syncthreads();
        for (int c = lane; c < (kc >> 4); c += 64) {
            float wf[L8_RW][16];
#pragma unroll
            for (int r = 0; r < L8_RW; ++r) i8x16_to_f32(load_nt16(wrow[r] + k0 + c * 16), wf[r]);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                float xf[16];
                Vec<T> x0, x1;
                x0.raw = xs[m * (L8_KC / 8) + 2 * c];
                x1.raw = xs[m * (L8_KC / 8) + 2 * c + 1];
                x0.to_float(*reinterpret_cast<float(*)[8]>(xf));
                x1.to_float(*reinterpret_cast<float(*)[8]>(xf + 8));
#pragma unroll
                for (int r = 0; r < L8_RW; ++r)
#pragma unroll
                    for (int j = 0; j < 16; ++j) acc[r][m] = fmaf(xf[j], wf[r][j], acc[r][m]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < L8_RW; ++r) {
        wave_sum_n<MT>(acc[r]);
        const int n = n0 + r;
        if (lane == 0 && n < N) {
            const float s = to_f(scale[n]), b = bias ? to_f(bias[n]) : 0.f;
#pragma unroll
            for (int m = 0; m < MT; ++m)
                if (m < M) out[(size_t)m * N + n] = from_f<T>(acc[r][m] * s + b);
        }
    }
}

// More rows: the register-staged 16-bit MFMA tile loop (gemm_tile_core.hip.h) with this B-side staging type, the int8 analogue
// of TileRegsFp8NT: one 16-byte load = 16 k of one weight row, converted exactly (no multiply) to 16 T on the way into LDS.
template <class T> __device__ __forceinline__ uint32_t pack16x2(float lo, float hi);
template <> __device__ __forceinline__ uint32_t pack16x2<bf16>(float lo, float hi) { return pack_bf16x2(lo, hi); }
template <> __device__ __forceinline__ uint32_t pack16x2<f16>(float lo, float hi) {
    return (uint32_t)__builtin_bit_cast(uint16_t, static_cast<_Float16>(lo)) | ((uint32_t)__builtin_bit_cast(uint16_t, static_cast<_Float16>(hi)) << 16);
}
template <int BN, class T>
struct TileRegsI8NT {
    static constexpr int CH = BN * 4 / GEMM_THREADS;   // 4 x 16-byte chunks per row of 64 k
    uint4 v[CH];
    __device__ __forceinline__ void load(const int8_t* w, int n0, int N, int k0, int K) {
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int c = threadIdx.x + i * GEMM_THREADS;
            const int gn = n0 + (c >> 2), gk = k0 + (c & 3) * 16;
            v[i] = gn < N && gk < K ? *reinterpret_cast<const uint4*>(w + (size_t)gn * K + gk) : make_uint4(0, 0, 0, 0);   // K % 16 == 0
        }
    }
    __device__ __forceinline__ void store(char* lds) const {
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int c = threadIdx.x + i * GEMM_THREADS;
            const int r = c >> 2, q = c & 3;
            float f[16];
            i8x16_to_f32(v[i], f);
            *reinterpret_cast<uint4*>(lds + swz128_off(r, q * 2)) =
                make_uint4(pack16x2<T>(f[0], f[1]), pack16x2<T>(f[2], f[3]), pack16x2<T>(f[4], f[5]), pack16x2<T>(f[6], f[7]));
            *reinterpret_cast<uint4*>(lds + swz128_off(r, q * 2 + 1)) =
                make_uint4(pack16x2<T>(f[8], f[9]), pack16x2<T>(f[10], f[11]), pack16x2<T>(f[12], f[13]), pack16x2<T>(f[14], f[15]));
        }
    }
};

template <class T, int BM>
__global__ __launch_bounds__(GEMM_THREADS) void linear_int8_mfma_kernel(const T* act, const int8_t* W, const T* scale, const T* bias, T* out,
                                                                       int M, int N, int K) {
    constexpr int BN = 128, WM = BM / 2, WN = BN / 2, TM = WM / 16, TN = WN / 16;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    TileRegsK<BM> ra;
    TileRegsI8NT<BN, T> rb;
    const int kbeg = 0, kend = K;
    auto load_tiles = [&](int k0) {
        ra.load(act, m0, M, k0, K, K);
        rb.load(W, n0, N, k0, K);
    };
    auto store_tiles = [&](int buf) {
        ra.store(gemm_tile_a<BM, BN>(smem, buf));
        rb.store(gemm_tile_b<BM, BN>(smem, buf));
    };
    f32x4_t acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#include "gemm_tile_loop.hip.h"      // the main loop: acc += act . W^T over [kbeg, kend)

    // C/D map of v_mfma_f32_16x16x32: col = lane & 15, row = (lane >> 4) * 4 + reg
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int col = n0 + wn * WN + j * 16 + (lane & 15);
            if (col >= N) continue;
            const float s = to_f(scale[col]), b = bias ? to_f(bias[col]) : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wm * WM + i * 16 + (lane >> 4) * 4 + r;
                if (row < M) out[(size_t)row * N + col] = from_f<T>(acc[i][j][r] * s + b);
            }
        }
}

// any K, any alignment: one output per thread
template <class T>
__global__ __launch_bounds__(256) void linear_int8_simple_kernel(const T* act, const int8_t* W, const T* scale, const T* bias, T* out, int M,
                                                                int N, int K, int ntn) {
    const int col = (int)(blockIdx.x % ntn) * 16 + (threadIdx.x & 15), row = (int)(blockIdx.x / ntn) * 16 + (threadIdx.x >> 4);
    if (row >= M || col >= N) return;
    const T* a = act + (size_t)row * K;
    const int8_t* w = W + (size_t)col * K;
    float acc = 0.f;
    for (int k = 0; k < K; ++k) acc = fmaf(to_f(a[k]), (float)w[k], acc);
    out[(size_t)row * N + col] = from_f<T>(acc * to_f(scale[col]) + (bias ? to_f(bias[col]) : 0.f));
}

template <class T>
static pgk_status launch_linear_int8(const void* act_, const int8_t* w, const void* scale_, const void* bias_, void* out_, int M, int N, int K,
                                     hipStream_t st) {
    const T* act = static_cast<const T*>(act_);
    const T* scale = static_cast<const T*>(scale_);
    const T* bias = static_cast<const T*>(bias_);
    T* out = static_cast<T*>(out_);
    switch (linear_int8_pick(M, K, aligned16(act) && aligned16(w))) {
        case L8_STREAM: {
            const unsigned grid = (unsigned)ceil_div(N, L8_ROWS);
            switch (linear_int8_stream_mt(M)) {
                case 1: linear_int8_stream_kernel<T, 1><<<grid, 256, 0, st>>>(act, w, scale, bias, out, M, N, K); break;
                case 2: linear_int8_stream_kernel<T, 2><<<grid, 256, 0, st>>>(act, w, scale, bias, out, M, N, K); break;
                case 4: linear_int8_stream_kernel<T, 4><<<grid, 256, 0, st>>>(act, w, scale, bias, out, M, N, K); break;
                default: linear_int8_stream_kernel<T, 8><<<grid, 256, 0, st>>>(act, w, scale, bias, out, M, N, K); break;
            }
            PGK_LAUNCH_CHECK();
            return PGK_OK;
        }
        case L8_MFMA: {
            PGK_REQUIRE(ceil_div(M, 64) <= 65535, "pgk_linear_int8: M=%d too large", M);
            if (M <= 64)
                return launch_dyn_lds<linear_int8_mfma_kernel<T, 64>>(dim3(ceil_div(N, 128), ceil_div(M, 64)), GEMM_THREADS, gemm_tile_lds_bytes(64, 128),
                                                                     true, st, act, w, scale, bias, out, M, N, K);
            return launch_dyn_lds<linear_int8_mfma_kernel<T, 128>>(dim3(ceil_div(N, 128), ceil_div(M, 128)), GEMM_THREADS, gemm_tile_lds_bytes(128, 128),
                                                                  true, st, act, w, scale, bias, out, M, N, K);
        }
        default: {
            const int ntn = ceil_div(N, 16);
            PGK_REQUIRE((long long)ntn * ceil_div(M, 16) < (1LL << 31), "pgk_linear_int8: M=%d N=%d too large", M, N);
            linear_int8_simple_kernel<T><<<(unsigned)(ntn * ceil_div(M, 16)), 256, 0, st>>>(act, w, scale, bias, out, M, N, K, ntn);
            PGK_LAUNCH_CHECK();
            return PGK_OK;
        }
    }
}

}  // namespace pgk

using namespace pgk;

extern "C" {

pgk_status pgk_gemm_int8_nt(const int8_t* a, const int8_t* b, int32_t* d, int m, int n, int k, pgk_stream s) {
    PGK_REQUIRE(a && b && d, "pgk_gemm_int8_nt: null argument");
    PGK_REQUIRE(m >= 1 && n >= 1 && k >= 1, "pgk_gemm_int8_nt: bad shape (m=%d n=%d k=%d)", m, n, k);
    return launch_int_gemm<IM_I8, EPI_I32, int32_t>(gemm_int8_pick(m, n, k, aligned16(a) && aligned16(b)), a, b, d, m, n, k, IntEpiArgs{},
                                                   resolve_stream(s));
}

pgk_status pgk_gemm_int8_dequant_nt(const int8_t* a, const float* a_scale, const int8_t* w, const float* w_scale, const void* bias, void* out,
                                    int m, int n, int k, pgk_dtype out_dt, pgk_stream s) {
    PGK_REQUIRE(a && a_scale && w && w_scale && out, "pgk_gemm_int8_dequant_nt: null argument");
    PGK_REQUIRE(m >= 1 && n >= 1 && k >= 1, "pgk_gemm_int8_dequant_nt: bad shape (m=%d n=%d k=%d)", m, n, k);
    const IntGemmKernel kern = gemm_int8_pick(m, n, k, aligned16(a) && aligned16(w));
    const IntEpiArgs e{a_scale, w_scale, bias, 1.f, 1.f, 1.f};
    hipStream_t st = resolve_stream(s);
    PGK_DISPATCH_FLOAT(out_dt, "pgk_gemm_int8_dequant_nt", return (launch_int_gemm<IM_I8, EPI_DEQUANT, T>(kern, a, w, (T*)out, m, n, k, e, st)));
    return PGK_OK;
}

pgk_status pgk_gemm_int4_nt(const uint8_t* a, const uint8_t* b, void* d, int m, int n, int k, float scale_a, float scale_b, float descale_d,
                            int out_int8, pgk_stream s) {
    PGK_REQUIRE(a && b && d, "pgk_gemm_int4_nt: null argument");
    PGK_REQUIRE(m >= 1 && n >= 1 && k >= 2 && k % 2 == 0, "pgk_gemm_int4_nt: k=%d must be positive and even (m=%d n=%d)", k, m, n);
    const IntGemmKernel kern = gemm_int4_pick(m, n, k, aligned16(a) && aligned16(b));
    const IntEpiArgs e{nullptr, nullptr, nullptr, scale_a, scale_b, descale_d};
    const bool planes = gemm_int4_plane_form(k), unit = scale_a == 1.0f && scale_b == 1.0f && descale_d == 1.0f;
    const int rb = k / 2;
    hipStream_t st = resolve_stream(s);
    if (out_int8) {
        if (planes) return launch_int_gemm<IM_I4_PLANES, EPI_SCALED, int8_t>(kern, a, b, (int8_t*)d, m, n, rb, e, st);
        return launch_int_gemm<IM_I4_EXT, EPI_SCALED, int8_t>(kern, a, b, (int8_t*)d, m, n, rb, e, st);
    }
    if (unit) {   // the accumulator itself: (float)acc would round it above 2^24
        if (planes) return launch_int_gemm<IM_I4_PLANES, EPI_I32, int32_t>(kern, a, b, (int32_t*)d, m, n, rb, e, st);
        return launch_int_gemm<IM_I4_EXT, EPI_I32, int32_t>(kern, a, b, (int32_t*)d, m, n, rb, e, st);
    }
    if (planes) return launch_int_gemm<IM_I4_PLANES, EPI_SCALED, int32_t>(kern, a, b, (int32_t*)d, m, n, rb, e, st);
    return launch_int_gemm<IM_I4_EXT, EPI_SCALED, int32_t>(kern, a, b, (int32_t*)d, m, n, rb, e, st);
}

pgk_status pgk_gemv_int4(const uint8_t* a, const uint8_t* b_nk, int32_t* c, int k, int n, float scale_a, float scale_b, pgk_stream s) {
    PGK_REQUIRE(a && b_nk && c, "pgk_gemv_int4: null argument");
    PGK_REQUIRE(n >= 1 && k >= 2 && k % 2 == 0, "pgk_gemv_int4: k=%d must be positive and even (n=%d)", k, n);
    hipStream_t st = resolve_stream(s);
    const int rb = k / 2;
    if (gemv_int4_pick(k, aligned16(a) && aligned16(b_nk)) == I4V_SIMPLE) {
        gemv_int4_simple_kernel<<<(unsigned)ceil_div(n, 4), 256, 0, st>>>(a, b_nk, c, n, rb, scale_a, scale_b);
    } else {
        switch (gemv_int4_rows_per_wave(k)) {
            case 4: gemv_int4_kernel<4><<<(unsigned)ceil_div(n, 16), 256, 0, st>>>(a, b_nk, c, n, rb, scale_a, scale_b); break;
            case 2: gemv_int4_kernel<2><<<(unsigned)ceil_div(n, 8), 256, 0, st>>>(a, b_nk, c, n, rb, scale_a, scale_b); break;
            default: gemv_int4_kernel<1><<<(unsigned)ceil_div(n, 4), 256, 0, st>>>(a, b_nk, c, n, rb, scale_a, scale_b); break;
        }
    }
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

pgk_status pgk_quantize_int8_rows(const void* x, int8_t* q, void* scale, int rows, int cols, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(x && q && scale, "pgk_quantize_int8_rows: null argument");
    PGK_REQUIRE(rows >= 1 && cols >= 1, "pgk_quantize_int8_rows: bad shape (rows=%d cols=%d)", rows, cols);
    hipStream_t st = resolve_stream(s);
    PGK_DISPATCH_FLOAT(dt, "pgk_quantize_int8_rows",
                       if (cols <= Q8_CACHED_COLS) quantize_int8_rows_kernel<T, true><<<(unsigned)rows, Q8_THREADS, 0, st>>>((const T*)x, q, (T*)scale, cols);
                       else quantize_int8_rows_kernel<T, false><<<(unsigned)rows, Q8_THREADS, 0, st>>>((const T*)x, q, (T*)scale, cols));
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

pgk_status pgk_dequantize_int8_rows(const int8_t* q, const void* scale, void* out, int rows, int cols, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(q && scale && out, "pgk_dequantize_int8_rows: null argument");
    PGK_REQUIRE(rows >= 1 && cols >= 1, "pgk_dequantize_int8_rows: bad shape (rows=%d cols=%d)", rows, cols);
    const size_t total = (size_t)rows * cols;
    PGK_REQUIRE(total / 256 < (1ull << 31), "pgk_dequantize_int8_rows: rows=%d cols=%d too large", rows, cols);
    hipStream_t st = resolve_stream(s);
    PGK_DISPATCH_FLOAT(dt, "pgk_dequantize_int8_rows",
                       dequantize_int8_rows_kernel<T><<<(unsigned)((total + 255) / 256), 256, 0, st>>>(q, (const T*)scale, (T*)out, total, cols));
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

pgk_status pgk_linear_int8(const void* act, const int8_t* w, const void* scale, const void* bias, void* out, int m, int n, int k, pgk_dtype dt,
                           pgk_stream s) {
    PGK_REQUIRE(act && w && scale && out, "pgk_linear_int8: null argument");
    PGK_REQUIRE(m >= 1 && n >= 1 && k >= 1, "pgk_linear_int8: bad shape (m=%d n=%d k=%d)", m, n, k);
    hipStream_t st = resolve_stream(s);
    switch (dt) {
        case PGK_F16: return launch_linear_int8<f16>(act, w, scale, bias, out, m, n, k, st);
        case PGK_BF16: return launch_linear_int8<bf16>(act, w, scale, bias, out, m, n, k, st);
        default: return set_error(PGK_ERR_INVALID, "pgk_linear_int8: dtype %d must be float16 or bfloat16", (int)dt);
    }
}

const char* pgk_int_gemm_plan(const char* op, int m, int n, int k, int aligned) {
    static thread_local char buf[64];
    const auto fail = [&](const char* why) -> const char* {
        set_error(PGK_ERR_INVALID, "pgk_int_gemm_plan: %s (op=%s M=%d N=%d K=%d)", why, op ? op : "NULL", m, n, k);
        return nullptr;
    };
    if (!op) return fail("null op");
    if (m < 1 || n < 1 || k < 1) return fail("bad shape");
    const std::string o(op);
    const bool al = aligned != 0;
    static const char* const tile[] = {"simple", "tile128", "tile64"};
    if (o == "gemm_int8" || o == "gemm_int8_dequant") {
        snprintf(buf, sizeof buf, "int8_%s", tile[gemm_int8_pick(m, n, k, al)]);
    } else if (o == "gemm_int4") {
        if (k % 2) return fail("K must be even");
        const IntGemmKernel kern = gemm_int4_pick(m, n, k, al);
        snprintf(buf, sizeof buf, "int4_%s%s", tile[kern], kern == IG_SIMPLE ? "" : gemm_int4_plane_form(k) ? "_planes" : "_ext");
    } else if (o == "gemv_int4") {
        if (k % 2) return fail("K must be even");
        if (gemv_int4_pick(k, al) == I4V_SIMPLE) return "gemv_int4_simple";
        snprintf(buf, sizeof buf, "gemv_int4_stream_r%d", gemv_int4_rows_per_wave(k));
    } else if (o == "linear_int8") {
        switch (linear_int8_pick(m, k, al)) {
            case L8_STREAM: snprintf(buf, sizeof buf, "linear_int8_stream_m%d", linear_int8_stream_mt(m)); break;
            case L8_MFMA: snprintf(buf, sizeof buf, "linear_int8_mfma_%d", m <= 64 ? 64 : 128); break;
            default: return "linear_int8_simple";
        }
    } else {
        return fail("unknown op");
    }
    return buf;
}

}  // extern "C"
