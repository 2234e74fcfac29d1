// Weight-streaming skinny MFMA GEMM for gfx950:  C[M,N] = A[M,K] . W[N,K]^T  with M <= 128.
//
// Prefill at S <= 128 (and batched decode) is WEIGHT-bound: 128 FLOP per weight byte vs the chip's 312, so
// the kernel is organised like the GEMV - every weight byte is read exactly once, straight from HBM into the
// MFMA B-operand registers - and not like a tiled GEMM:
//   * a wave owns one 16-row slab of W and walks K; lane l loads W[n0 + (l&15)][k + 8*(l>>4) .. +8], which IS the
//     B fragment of v_mfma_f32_16x16x32_bf16 (no LDS round trip for the read-once operand); 8 k-steps of loads
//     are in flight per wave before the first is consumed;
//   * the activations (the re-used operand) sit in LDS as [M_pad][256] K-tiles, XOR-swizzled so the 16 rows of an
//     A-fragment read hit 16 different 16-byte slots; one fragment read feeds MT = M_pad/16 MFMAs;
//   * fp32 accumulators stay in registers across the whole K range of the workgroup;
//   * small-N projections (N = hidden) are split along K over workgroups so the whole chip streams; partial
//     results go to fp32 slabs that the consumer (the next RMSNorm) sums - deterministic, no atomics.
// The reference has nothing of this shape (M < 16 goes to cuBLASLt, M >= 16 to 128x128 CUTLASS tiles,
// native/ops/matmul/matmul.cu:142-235).

// The walk itself is wsgemm_core.hip.h (shared with the grouped expert GEMM); this file has the dense problem, the three
// epilogues and the launcher.

#include "gemm_plan.h"
#include "pgk_internal.h"
#include "wsgemm_core.hip.h"

namespace pgk {

struct WsArgs {
    const bf16* a;      // [M][lda]
    int lda;
    const void* w;      // [N][K] bf16, or fp8 codes with wscale
    const bf16* wscale; // fp8: [N/128][K/128]
    int M, N, K;
    int k_per_split;    // multiple of WS_KT
    void* c;            // mode 0: bf16 [M][N]; mode 1: fp32 slabs [ksplits][M][N]; mode 2: fp32 [M][N] += (ksplits == 1)
    const bf16* bias;   // mode 0 only
    int mode;
};

// the problem of wsgemm_walk: rows of one matrix, K split over blockIdx.y
struct WsDense {
    const bf16* a;
    int lda;
    const void* w;
    const bf16* wscale;
    int M, N, K, kbeg, kend;
    __device__ __forceinline__ const bf16* a_row(int r) const { return a + (size_t)min(r, M - 1) * lda; }
};

template <int MT, bool FP8, int MODE>
__global__ __launch_bounds__(WS_THREADS) void wsgemm_kernel(WsArgs g) {
    extern __shared__ __attribute__((aligned(16))) char a_lds[];   // [MT*16][256] bf16, swizzled
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int n0 = (blockIdx.x * 4 + wid) * 16;
    const int kbeg = blockIdx.y * g.k_per_split;
    const WsDense p{g.a, g.lda, g.w, g.wscale, g.M, g.N, g.K, kbeg, min(kbeg + g.k_per_split, g.K)};

    f32x4_t acc[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) acc[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    wsgemm_walk<MT, FP8, false, true>(p, a_lds, n0, acc);      // no row tile to skip; A fragments read ahead

    // C/D map: col (n) = lane & 15, row (m) = (lane >> 4) * 4 + reg.  Straight-line epilogue: the bias /
    // read-modify-write loads are issued together, never one per element under a branch.
    const int n = min(n0 + (lane & 15), g.N - 1);
    const bool n_ok = n0 + (lane & 15) < g.N;
    if constexpr (MODE == 0) {
        const float b = g.bias ? to_f(g.bias[n]) : 0.f;
        bf16* c = reinterpret_cast<bf16*>(g.c);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = mt * 16 + (lane >> 4) * 4 + r;
                if (n_ok && m < g.M) c[(size_t)m * g.N + n] = from_f<bf16>(acc[mt][r] + b);
            }
    } else if constexpr (MODE == 1) {
        float* c = reinterpret_cast<float*>(g.c) + (size_t)blockIdx.y * g.M * g.N;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = mt * 16 + (lane >> 4) * 4 + r;
                if (n_ok && m < g.M) c[(size_t)m * g.N + n] = acc[mt][r];
            }
    } else {
        float* c = reinterpret_cast<float*>(g.c);
        float old[MT][4];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) old[mt][r] = c[(size_t)min(mt * 16 + (lane >> 4) * 4 + r, g.M - 1) * g.N + n];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = mt * 16 + (lane >> 4) * 4 + r;
                if (n_ok && m < g.M) c[(size_t)m * g.N + n] = old[mt][r] + acc[mt][r];
            }
    }
}

// MT x FP8 x mode -> the instantiation; its LDS limit is raised (once) where MT*16 rows of 512 bytes pass 48 KiB
template <int MT, bool FP8>
static pgk_status wsgemm_launch_mode(const WsArgs& g, dim3 grid, hipStream_t st) {
    constexpr size_t lds = ws_lds_bytes(MT);
    constexpr bool raise = lds > 48 * 1024;
    if (g.mode == 0) return launch_dyn_lds<&wsgemm_kernel<MT, FP8, 0>>(grid, WS_THREADS, lds, raise, st, g);
    if (g.mode == 1) return launch_dyn_lds<&wsgemm_kernel<MT, FP8, 1>>(grid, WS_THREADS, lds, raise, st, g);
    return launch_dyn_lds<&wsgemm_kernel<MT, FP8, 2>>(grid, WS_THREADS, lds, raise, st, g);
}
template <int MT>
static pgk_status wsgemm_launch(const WsArgs& g, bool fp8, dim3 grid, hipStream_t st) {
    return fp8 ? wsgemm_launch_mode<MT, true>(g, grid, st) : wsgemm_launch_mode<MT, false>(g, grid, st);
}

// A[M,K] bf16 (row stride lda), W[N,K]; mode 0: bf16 C (+bias); mode 1: fp32 slabs [splits][M][N]; mode 2: fp32 C += .
pgk_status wsgemm_nt(const bf16* a, int lda, const void* w, const bf16* wscale, bool fp8, void* c, const bf16* bias, int mode,
                     int splits, int M, int N, int K, hipStream_t st) {
    PGK_REQUIRE(M >= 1 && M <= 128, "wsgemm: M=%d outside [1,128]", M);
    PGK_REQUIRE(K % 8 == 0 && lda % 8 == 0, "wsgemm: K=%d / lda=%d must be multiples of 8", K, lda);
    PGK_REQUIRE(mode == 1 || splits == 1, "wsgemm: split-K needs slab output");
    WsArgs g{a, lda, w, wscale, M, N, K, 0, c, bias, mode};
    int kps = ceil_div(K, splits);
    kps = ceil_div(kps, WS_KT) * WS_KT;
    g.k_per_split = kps;
    const int real_splits = ceil_div(K, kps);
    PGK_REQUIRE(real_splits == splits, "wsgemm: %d splits do not tile K=%d (use %d)", splits, K, real_splits);
    const int mt = wsgemm_pick_mt(M);      // gemm_plan.h: 1, 2, 4 or 8 tiles of 16 rows
    dim3 grid(ceil_div(N, 64), splits);
    switch (mt) {
        case 1: return wsgemm_launch<1>(g, fp8, grid, st);
        case 2: return wsgemm_launch<2>(g, fp8, grid, st);
        case 4: return wsgemm_launch<4>(g, fp8, grid, st);
        case 8: return wsgemm_launch<8>(g, fp8, grid, st);
    }
    return set_error(PGK_ERR_INVALID, "wsgemm: no tile for M=%d", M);
}

}  // namespace pgk
