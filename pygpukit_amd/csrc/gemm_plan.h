// Host-side kernel choice of the dense GEMM family: pgk_gemm_nt, pgk_gemm_nn, pgk_w8a16_gemm_nk / _kn, pgk_gemv_fp8_bf16 and
// pgk_gemm_fp8_nt.  Every `if` ladder of those dispatchers lives here as a pure function of the shape (plus PGK_GEMM256 /
// PGK_GEMM256S, read per call); the launchers switch on what these functions return and pgk_gemm_plan (ops_gemm.hip) prints
// the same return values, so the plan query cannot drift from the dispatch.  No device, stream or pointer is touched here.
#pragma once

#include <cstdlib>

#include "pgk_internal.h"

namespace pgk {

bool want_gemm256(int M, int N);          // ops_gemm.hip: enough 256 x 256 tiles to fill the chip, or PGK_GEMM256 = 0 / 1
bool gemm128s_ok(int M, int N, int K);    // ops_gemm256.hip: the shapes of the staged 128 x 128 kernel

inline bool use_gemm256(int M, int N, int K) { return K % 64 == 0 && want_gemm256(M, N); }

// ---- launch_gemv (ops_gemv.hip): activations staged in LDS and 16-byte weight loads, or the element-wise kernel ------------
enum GemvKernel { GEMV_FAST = 0, GEMV_GENERIC = 1 };
inline GemvKernel gemv_pick(int M, int K, size_t elem_size, bool ptrs_aligned) {
    const int nv = (int)(16 / elem_size);
    const size_t lds = (size_t)M * K * elem_size;
    return (K % nv == 0) && ptrs_aligned && lds <= 64 * 1024 && M <= 8 ? GEMV_FAST : GEMV_GENERIC;
}

// ---- wsgemm_nt (ops_wsgemm.hip): M tiles of 16 rows held per workgroup, 1 / 2 / 4 / 8 (0: M > 128, no kernel) --------------
inline int wsgemm_pick_mt(int M) {
    const int mt = ceil_div(M, 16);
    return mt <= 1 ? 1 : mt <= 2 ? 2 : mt <= 4 ? 4 : mt <= 8 ? 8 : 0;
}

// ---- gemm256_bf16_nt (ops_gemm256.hip) ---------------------------------------------------------------------------------------
enum Gemm256Kernel { G256_STAGGERED = 0, G256_STAGGERED_N192 = 1, G256_LOCKSTEP = 2 };
inline Gemm256Kernel gemm256_pick(int M, int N, bool accum_f32, bool packed) {
    const int ntm = ceil_div(M, 256), ntn = ceil_div(N, 256);
    const char* e = getenv("PGK_GEMM256S");          // 0: two full stages, waves in lockstep; default: staggered phases
    if (!(packed || !e || atoi(e) != 0)) return G256_LOCKSTEP;
    // 192-column tiles when they fill the rounds of the chip better (cost = rounds x work per tile)
    const int ntn3 = N / 192;
    const bool narrow = !accum_f32 && N % 192 == 0 &&
                        0.75 * ceil_div(ntm * ntn3, 256) < (double)ceil_div(ntm * ntn, 256) - 0.01;
    return narrow ? G256_STAGGERED_N192 : G256_STAGGERED;
}

// ---- dispatch_mfma (ops_gemm.hip): smallest BM covering M (<= 128); BN as large as keeps >= ~256 workgroups in flight --------
struct MfmaTile { int bm, bn; };
inline MfmaTile mfma_pick_tile(int M, int N, bool b_kn_fp8) {
    int bm = M <= 32 ? 32 : (M <= 64 ? 64 : 128);
    long long mblocks = (M + bm - 1) / bm;
    int bn = 128;
    while (bn > 32 && mblocks * ((N + bn - 1) / bn) < 256) bn >>= 1;
    // 128 x 64 tiles that only just cover the chip (one 4-wave workgroup per CU, nothing to overlap its barriers with)
    // lose to twice as many 64 x 64 tiles: M=2048, N=1024, K=2048/3072 measured 23.9 / 33.9 us against 28.3 / 39.9
    if (bm == 128 && bn == 64 && mblocks * ((N + 63) / 64) < 512) { bm = 64; mblocks = (M + 63) / 64; }
    if (b_kn_fp8 && bn < 64) bn = 64;  // keep whole 16-code chunks per thread
    return {bm, bn};
}

// ---- pgk_gemm_nt ---------------------------------------------------------------------------------------------------------------
enum GemmNtKernel { NT_GEMV = 0, NT_SIMPLE, NT_WSGEMM, NT_GEMM256, NT_GEMM128S, NT_MFMA };
// ptrs_aligned: A and W on 16-byte boundaries
inline GemmNtKernel gemm_nt_pick(int m, int n, int k, pgk_dtype dt, bool ptrs_aligned) {
    const bool al = ptrs_aligned && (k % 8 == 0);
    if (dt == PGK_F32 || !al) return m <= 8 ? NT_GEMV : NT_SIMPLE;
    if (m <= 8 && (size_t)m * k * 2 <= 64 * 1024) return NT_GEMV;     // weight-streaming GEMV path
    if (dt == PGK_BF16 && m <= 128) return NT_WSGEMM;                 // weight-bound regime: stream W once through the skinny MFMA kernel
    if (dt == PGK_BF16 && use_gemm256(m, n, k)) return NT_GEMM256;
    if (dt == PGK_BF16 && gemm128s_ok(m, n, k)) return NT_GEMM128S;
    return NT_MFMA;
}

// ---- pgk_gemm_nn ---------------------------------------------------------------------------------------------------------------
enum GemmNnKernel { NN_SIMPLE = 0, NN_MFMA };
inline GemmNnKernel gemm_nn_pick(int n, int k, pgk_dtype dt, bool ptrs_aligned) {
    const bool al = ptrs_aligned && (k % 8 == 0) && (n % 8 == 0);
    return dt == PGK_F32 || !al ? NN_SIMPLE : NN_MFMA;
}

// ---- pgk_w8a16_gemm_nk (and the fp8-weight branch of engine_gemm_nt behind it) -----------------------------------------------
enum W8a16NkKernel { W8_WSGEMM = 0, W8_DEQUANT_GEMM256, W8_MFMA };
// M > 128: dequantise the weight once and run the LDS-DMA bf16 kernel, or dequantise in the staging path of the 128-tile kernel
inline W8a16NkKernel w8a16_large_pick(int M, int N, int K) {
    return use_gemm256(M, N, K) && K % 128 == 0 && N % 128 == 0 ? W8_DEQUANT_GEMM256 : W8_MFMA;
}
inline W8a16NkKernel w8a16_nk_pick(int m, int n, int k) { return m <= 128 ? W8_WSGEMM : w8a16_large_pick(m, n, k); }

// ---- pgk_gemv_fp8_bf16: M rows in passes of <= 8 (weights are re-read per pass) ----------------------------------------------
inline int gemv_fp8_pass_rows(int m, int m0) { return (m - m0) < 8 ? (m - m0) : 8; }

// ---- gemm_fp8_nt (ops_fp8_gemm.hip) --------------------------------------------------------------------------------------------
enum GemmFp8Kernel { FP8_TILE128 = 0, FP8_TILE256 };
// enough 256 x 256 tiles to fill the chip: the LDS-DMA structure (ops_gemm256.hip), whole tiles only
inline GemmFp8Kernel gemm_fp8_pick(int M, int N) {
    return want_gemm256(M, N) && M % 256 == 0 && N % 256 == 0 ? FP8_TILE256 : FP8_TILE128;
}

}  // namespace pgk
