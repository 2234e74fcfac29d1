// fp8-in / fp8-out GEMM on a row-major [K,N] B operand (matmul_fp8_fp8_sm120 and its blockwise form,
// src/pygpukit/ops/matmul/fp8.py:220-343):
//
//   D[m][n] = e4m3( sum_kb  sA(m/128, kb) * sB(n/128, kb) * sum_{k in block kb} A[m][k] * B[k][n] )
//
//   A [M,K], B [K,N], D [M,N]: OCP e4m3 codes, all row-major as their shapes say.
//   scale_a / scale_b fp32, one per 128x128 block, MN-major: (mb, kb) at kb * ceil(M/128) + mb, (nb, kb) at
//   kb * ceil(N/128) + nb (CUTLASS's Sm1xxBlockwiseScaleConfig default; see include/pgk_hip.h).  Both NULL: unit
//   scales - the MFMA accumulates in its own C operand, no scale loads.
//
// One workgroup = 128x128 outputs, 4 waves as 2x2 of 64x64, 128-deep k steps, so a workgroup sits inside one
// (mb, nb) scale block and the scale product is one scalar per k step.  The inner sum of one k step is one
// v_mfma_scale_f32_16x16x128_f8f6f4 per 16x16 output tile (as gemm_fp8_kernel, ops_fp8_gemm.hip).
//
// The fp8 MFMA B fragment wants 32 consecutive k of one column per lane, while consecutive bytes of a [K,N] row run
// along n.  The transpose happens in the register-staging write pass: each thread loads an 8(k) x 8(n) byte block
// (8-byte loads, 16 lanes cover 128 contiguous bytes of a row), transposes it with v_perm_b32 and writes eight
// 8-byte k-runs into a [n][k] LDS image - the image gemm_fp8_kernel builds from an [N,K] weight, read the same way.
// No transposed copy of B exists in global memory.
//
// K need not be a multiple of 128: bytes past K are staged as 0x00 (+0).  Rows past M read row M-1 (never
// stored), columns past N read a valid column (never stored).
//
// Output: fp32 -> e4m3 round-to-nearest-even with satfinite (|x| > 448 -> +-448, 0x7E / 0xFE), NaN kept as a NaN
// code, -0 -> 0x80; the 128x128 byte tile goes through LDS so that D is written with 16-byte stores.

#include "mfma_common.hip.h"
#include "pgk_device.hip.h"
#include "pgk_internal.h"

namespace pgk {

constexpr int NN_BM = 128, NN_BN = 128, NN_BK = 128, NN_THREADS = 256;
constexpr int NN_TILE = 128 * 128;   // bytes of one staged operand tile

// A image [128 m][128 k] and the D tile: 16-byte chunk kc of row r at r*128 + 16*(kc ^ (r & 7)) (gemm_fp8_kernel's)
__device__ __forceinline__ int nn_off_a(int row, int kc) { return row * 128 + ((kc ^ (row & 7)) << 4); }
// B image [128 n][128 k]: the XOR key also takes row >> 3.  In the write pass the 16 lanes of one k-run write rows 8
// apart; with key (row & 7) they would all hit the same 16 bytes of a bank line.
__device__ __forceinline__ int nn_off_b(int row, int kc) { return row * 128 + ((kc ^ ((row ^ (row >> 3)) & 7)) << 4); }

// 4x4 byte transpose: in x_r byte j = T[r][j]; out y_j byte r = T[r][j].
// v_perm_b32(s0, s1, sel): byte selector 0..3 picks s1's bytes, 4..7 s0's.
__device__ __forceinline__ void nn_tr4(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3, uint32_t& y0, uint32_t& y1,
                                       uint32_t& y2, uint32_t& y3) {
    const uint32_t p01l = __builtin_amdgcn_perm(x1, x0, 0x05010400u);   // x0b0 x1b0 x0b1 x1b1
    const uint32_t p01h = __builtin_amdgcn_perm(x1, x0, 0x07030602u);   // x0b2 x1b2 x0b3 x1b3
    const uint32_t p23l = __builtin_amdgcn_perm(x3, x2, 0x05010400u);
    const uint32_t p23h = __builtin_amdgcn_perm(x3, x2, 0x07030602u);
    y0 = __builtin_amdgcn_perm(p23l, p01l, 0x05040100u);
    y1 = __builtin_amdgcn_perm(p23l, p01l, 0x07060302u);
    y2 = __builtin_amdgcn_perm(p23h, p01h, 0x05040100u);
    y3 = __builtin_amdgcn_perm(p23h, p01h, 0x07060302u);
}

// satfinite clamp that keeps NaN (fminf/fmaxf alone would turn NaN into +-448); the conversion itself is RNE
__device__ __forceinline__ float nn_satfinite(float x) { return __builtin_isnan(x) ? x : fminf(fmaxf(x, -448.0f), 448.0f); }

// amdgpu_waves_per_eu(2): two workgroups per CU (the blockwise fold would otherwise take the register file to one)
template <bool UNIT>
__global__ __launch_bounds__(NN_THREADS) __attribute__((amdgpu_waves_per_eu(2))) void gemm_fp8_fp8_nn_kernel(const uint8_t* __restrict__ A, const uint8_t* __restrict__ B,
                                                                     uint8_t* __restrict__ D, const float* __restrict__ sa,
                                                                     const float* __restrict__ sb, int M, int N, int K) {
    extern __shared__ __attribute__((aligned(16))) char smem[];   // A[2] | B[2]
    auto As = [&](int buf) -> char* { return smem + buf * NN_TILE; };
    auto Bs = [&](int buf) -> char* { return smem + 2 * NN_TILE + buf * NN_TILE; };

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1, q = lane >> 4;
    const int m0 = blockIdx.y * NN_BM, n0 = blockIdx.x * NN_BN;
    const int KT = (K + NN_BK - 1) / NN_BK;
    const int MB = gridDim.y, NB = gridDim.x;

    // A staging: 4 rows x 16 B (rows srow + 32 i, chunk skc), as gemm_fp8_kernel
    const int srow = tid >> 3, skc = tid & 7;
    const uint8_t* a_p0 = A + (size_t)min(m0 + srow, M - 1) * K + skc * 16;
    const uint8_t* a_p1 = A + (size_t)min(m0 + 32 + srow, M - 1) * K + skc * 16;
    const uint8_t* a_p2 = A + (size_t)min(m0 + 64 + srow, M - 1) * K + skc * 16;
    const uint8_t* a_p3 = A + (size_t)min(m0 + 96 + srow, M - 1) * K + skc * 16;
    const int a_st = nn_off_a(srow, skc);   // rows srow + 32 i share the swizzle (32 % 8 == 0)
    // B staging: k rows 8 kg .. 8 kg + 7 of the k step, columns 8 ng .. 8 ng + 7 of the tile (N % 16 == 0, so an
    // 8-byte run is wholly inside or wholly past N; past N it reads the last run, never stored)
    const int ng = tid & 15, kg = tid >> 4;
    const uint8_t* b_p = B + (size_t)(kg * 8) * N + min(n0 + ng * 8, N - 8);
    const size_t b_step = (size_t)NN_BK * N;

    // named staging registers, not arrays: hipcc can leave a staging array in scratch memory
    uint4 ra0, ra1, ra2, ra3;
    uint2 rb0, rb1, rb2, rb3, rb4, rb5, rb6, rb7;
    float s_next = 1.0f;
    auto load_tiles = [&](int kt) {
        const size_t ka = (size_t)kt * NN_BK;
        const uint8_t* bp = b_p + (size_t)kt * b_step;
        if (kt * NN_BK + NN_BK <= K) {
            ra0 = *reinterpret_cast<const uint4*>(a_p0 + ka); ra1 = *reinterpret_cast<const uint4*>(a_p1 + ka);
            ra2 = *reinterpret_cast<const uint4*>(a_p2 + ka); ra3 = *reinterpret_cast<const uint4*>(a_p3 + ka);
            rb0 = *reinterpret_cast<const uint2*>(bp + 0 * (size_t)N); rb1 = *reinterpret_cast<const uint2*>(bp + 1 * (size_t)N);
            rb2 = *reinterpret_cast<const uint2*>(bp + 2 * (size_t)N); rb3 = *reinterpret_cast<const uint2*>(bp + 3 * (size_t)N);
            rb4 = *reinterpret_cast<const uint2*>(bp + 4 * (size_t)N); rb5 = *reinterpret_cast<const uint2*>(bp + 5 * (size_t)N);
            rb6 = *reinterpret_cast<const uint2*>(bp + 6 * (size_t)N); rb7 = *reinterpret_cast<const uint2*>(bp + 7 * (size_t)N);
        } else {   // the last, partial k step: chunks / rows at or past K are +0 (K % 16 == 0: a 16-byte A chunk is all in or all out)
            const int left = K - kt * NN_BK;
            const bool ain = skc * 16 < left;
            const int kr = kg * 8;
            auto lda = [&](const uint8_t* p) { uint4 v = make_uint4(0, 0, 0, 0); if (ain) v = *reinterpret_cast<const uint4*>(p + ka); return v; };
            auto ldb = [&](int r) { uint2 v = make_uint2(0, 0); if (kr + r < left) v = *reinterpret_cast<const uint2*>(bp + r * (size_t)N); return v; };
            ra0 = lda(a_p0); ra1 = lda(a_p1); ra2 = lda(a_p2); ra3 = lda(a_p3);
            rb0 = ldb(0); rb1 = ldb(1); rb2 = ldb(2); rb3 = ldb(3); rb4 = ldb(4); rb5 = ldb(5); rb6 = ldb(6); rb7 = ldb(7);
        }
        if constexpr (!UNIT) s_next = sa[(size_t)kt * MB + blockIdx.y] * sb[(size_t)kt * NB + blockIdx.x];
    };
    auto store_tiles = [&](int buf) {
        char* a = As(buf) + a_st;
        *reinterpret_cast<uint4*>(a) = ra0; *reinterpret_cast<uint4*>(a + 32 * 128) = ra1;
        *reinterpret_cast<uint4*>(a + 64 * 128) = ra2; *reinterpret_cast<uint4*>(a + 96 * 128) = ra3;
        // rows 0..3 / 4..7 of the 8x8 block -> k bytes 0..3 / 4..7 of each of the 8 columns
        uint32_t lo[8], hi[8];
        nn_tr4(rb0.x, rb1.x, rb2.x, rb3.x, lo[0], lo[1], lo[2], lo[3]);
        nn_tr4(rb0.y, rb1.y, rb2.y, rb3.y, lo[4], lo[5], lo[6], lo[7]);
        nn_tr4(rb4.x, rb5.x, rb6.x, rb7.x, hi[0], hi[1], hi[2], hi[3]);
        nn_tr4(rb4.y, rb5.y, rb6.y, rb7.y, hi[4], hi[5], hi[6], hi[7]);
        char* b = Bs(buf);
#pragma unroll
        for (int j = 0; j < 8; ++j)   // column ng*8 + j: key ((ng*8 + j) ^ ng) & 7 = (j ^ ng) & 7
            *reinterpret_cast<uint2*>(b + nn_off_b(ng * 8 + j, kg >> 1) + 8 * (kg & 1)) = make_uint2(lo[j], hi[j]);
    };

    f32x4_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    load_tiles(0);
    store_tiles(0);
    float s_cur = s_next;
    __syncthreads();
    for (int kt = 0; kt < KT; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < KT) load_tiles(kt + 1);
        auto frag = [&](const char* tile, int row, bool b_image) -> i32x8_t {   // 32 k of one row: k = 32 q .. 32 q + 31
            const uint4 x0 = *reinterpret_cast<const uint4*>(tile + (b_image ? nn_off_b(row, 2 * q) : nn_off_a(row, 2 * q)));
            const uint4 x1 = *reinterpret_cast<const uint4*>(tile + (b_image ? nn_off_b(row, 2 * q + 1) : nn_off_a(row, 2 * q + 1)));
            return i32x8_t{(int)x0.x, (int)x0.y, (int)x0.z, (int)x0.w, (int)x1.x, (int)x1.y, (int)x1.z, (int)x1.w};
        };
        i32x8_t fb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) fb[j] = frag(Bs(buf), wn * 64 + j * 16 + (lane & 15), true);
        if constexpr (UNIT) {
            i32x8_t fa[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) fa[i] = frag(As(buf), wm * 64 + i * 16 + (lane & 15), false);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fa[i], fb[j], acc[i][j], 0, 0, 0, 0, 0, 0);
        } else {
            // per row i of tiles: its A fragment, 4 zero-C MFMAs, then the fold of row i - 1 behind them.  Two rows of
            // products and one A fragment live at a time; all 16 products in flight would cost the second wave per SIMD.
            f32x4_t tp[4], tc[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const i32x8_t fa = frag(As(buf), wm * 64 + i * 16 + (lane & 15), false);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    tc[j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fa, fb[j], f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0, 0, 0, 0);
                if (i > 0) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i - 1][j] += tp[j] * s_cur;
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < 4; ++j) tp[j] = tc[j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[3][j] += tp[j] * s_cur;
        }
        if (kt + 1 < KT) {
            store_tiles(buf ^ 1);
            s_cur = s_next;
        }
        __syncthreads();
    }

    // epilogue: e4m3 codes into a [128][128] byte tile in LDS (the loop's last barrier has retired every read of As(0)),
    // then 16-byte rows out (measured against one global byte store per code: equal or up to 5 % faster,
    // profiles/r04_fp8nn_gemm_bench.log).  C/D map of the 16x16 MFMA: col = lane & 15, row = (lane >> 4) * 4 + reg.
    char* dt = As(0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f32x4_t v = acc[i][j];
            const uint32_t w = pack_fp8x4(nn_satfinite(v[0]), nn_satfinite(v[1]), nn_satfinite(v[2]), nn_satfinite(v[3]));
            const int col = wn * 64 + j * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = wm * 64 + i * 16 + q * 4 + r;
                dt[nn_off_a(row, col >> 4) + (col & 15)] = (char)(w >> (8 * r));
            }
        }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int row = p * 32 + srow, grow = m0 + row, gcol = n0 + skc * 16;
        if (grow < M && gcol < N)
            *reinterpret_cast<uint4*>(D + (size_t)grow * N + gcol) = *reinterpret_cast<const uint4*>(dt + nn_off_a(row, skc));
    }
}

pgk_status gemm_fp8_fp8_nn(const uint8_t* a, const uint8_t* b, uint8_t* d, const float* sa, const float* sb, int M, int N, int K,
                           hipStream_t st) {
    constexpr size_t LDS = 4 * (size_t)NN_TILE;
    static bool attr_done = false;
    if (!attr_done) {
        PGK_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_fp8_fp8_nn_kernel<true>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS));
        PGK_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_fp8_fp8_nn_kernel<false>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS));
        attr_done = true;
    }
    // grid.y / grid.x are ceil(M/128) / ceil(N/128): the kernel reads them as the scale arrays' MN extents
    const dim3 grid(ceil_div(N, NN_BN), ceil_div(M, NN_BM));
    if (sa) gemm_fp8_fp8_nn_kernel<false><<<grid, NN_THREADS, LDS, st>>>(a, b, d, sa, sb, M, N, K);
    else gemm_fp8_fp8_nn_kernel<true><<<grid, NN_THREADS, LDS, st>>>(a, b, d, nullptr, nullptr, M, N, K);
    PGK_CHECK_HIP(hipGetLastError());
    return PGK_OK;
}

}  // namespace pgk

using namespace pgk;

extern "C" {

pgk_status pgk_gemm_fp8_fp8_nn(const uint8_t* a_mk, const uint8_t* b_kn, uint8_t* d_mn, const float* scale_a, const float* scale_b,
                               int m, int n, int k, pgk_stream s) {
    PGK_REQUIRE(a_mk && b_kn && d_mn, "pgk_gemm_fp8_fp8_nn: null operand");
    PGK_REQUIRE((scale_a == nullptr) == (scale_b == nullptr),
                "pgk_gemm_fp8_fp8_nn: scale_a and scale_b must both be given or both be NULL (unit scales)");
    PGK_REQUIRE(m >= 1 && n >= 16 && k >= 16 && n % 16 == 0 && k % 16 == 0,
                "pgk_gemm_fp8_fp8_nn: bad shape M=%d N=%d K=%d (M >= 1; N and K positive multiples of 16)", m, n, k);
    PGK_REQUIRE(aligned16(a_mk) && aligned16(b_kn) && aligned16(d_mn), "pgk_gemm_fp8_fp8_nn: operands must be 16-byte aligned");
    return gemm_fp8_fp8_nn(a_mk, b_kn, d_mn, scale_a, scale_b, m, n, k, resolve_stream(s));
}

}  // extern "C"
