// Host-side kernel choice of the dense GEMM family: pgk_gemm_nt, pgk_gemm_nn, pgk_w8a16_gemm_nk / _kn, pgk_gemv_fp8_bf16 and
// pgk_gemm_fp8_nt, and of the grouped expert GEMM pgk_grouped_gemm_sorted (regime, K splits, row tiles: pgk_grouped_gemm_sorted_splits
// is its query).  Every `if` ladder of those dispatchers lives here as a pure function of the shape (plus PGK_GEMM256 /
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

// K splits (fp32 slabs for the consumer to sum) so that ~256+ workgroups stream; normalised to a count that tiles K in whole
// LDS tiles, which is what wsgemm_nt launches.
constexpr int WS_KT = 256;        // K elements per LDS tile of the weight-streaming walk (wsgemm_core.hip.h)
inline int ws_whole_tile_splits(int K, int s) {
    const int kps = ceil_div(ceil_div(K, s), WS_KT) * WS_KT;
    return ceil_div(K, kps);
}
inline int wsgemm_pick_splits(int N, int K, bool allow_split) {
    const int nblk = ceil_div(N, 64);
    if (!allow_split || nblk >= 192) return 1;
    int s = ceil_div(256, nblk);
    const int max_s = K / WS_KT;
    if (s > max_s) s = max_s;
    if (s > 16) s = 16;
    if (s < 1) s = 1;
    return ws_whole_tile_splits(K, s);
}

// ---- pgk_grouped_gemm_sorted (ops_moe.hip) -----------------------------------------------------------------------------------
constexpr int MOE_TILE_ROWS = 128;      // rows per tile-table entry (both grouped-GEMM regimes)
constexpr int MOE_WS_ROWS_MAX = 64;     // T*k/E at or below this: weight-streaming regime, above: 128 x 128 tiles
inline int moe_max_tiles(int T, int k, int E) { return ceil_div((long long)T * k, MOE_TILE_ROWS) + E; }
inline bool moe_ws_regime(int T, int k, int E) { return (long long)T * k <= (long long)MOE_WS_ROWS_MAX * E; }
// K splits of the weight-streaming regime: enough (expected active expert, 64-column slab, split) workgroups to stream on
// every CU.  1 in the tiled regime.
inline int moe_sorted_splits(int T, int k, int E, int N, int K) {
    if (!moe_ws_regime(T, k, E)) return 1;
    const long long active = E < (long long)T * k ? E : (long long)T * k;
    const long long wgs = active * ceil_div(N, 64);
    int s = wgs >= 512 ? 1 : ceil_div(512, wgs);
    const int max_s = K / WS_KT < 1 ? 1 : K / WS_KT;
    if (s > max_s) s = max_s;
    if (s > 16) s = 16;
    return ws_whole_tile_splits(K, s);
}
// row tiles of 16 the weight-streaming kernel holds: no expert can have more rows than there are, or than a table entry
inline int moe_ws_pick_mt(int T, int k) {
    const long long rows = (long long)T * k;
    return wsgemm_pick_mt((int)(rows < MOE_TILE_ROWS ? rows : MOE_TILE_ROWS));
}

// ---- gemm256_bf16_nt / gemm256_bf16_swiglu_nt (ops_gemm256.hip) --------------------------------------------------------------
// Narrower tiles (three quarters of the columns: `ntn_narrow` of them where there were `ntn`) when they fill the rounds of the
// chip better (cost = rounds x work per tile): Qwen3-0.6B's gate / up at S = 2048 is 8 x 24 = 192 tiles of 128 act columns
// (three quarters of the CUs, one round) or 8 x 32 = 256 tiles of 96 (all of them).
inline bool gemm256_narrow_fills_better(int ntm, int ntn, int ntn_narrow) {
    return 0.75 * ceil_div(ntm * ntn_narrow, 256) < (double)ceil_div(ntm * ntn, 256) - 0.01;
}
enum Gemm256Kernel { G256_STAGGERED = 0, G256_STAGGERED_N192 = 1, G256_LOCKSTEP = 2 };
inline Gemm256Kernel gemm256_pick(int M, int N, bool accum_f32, bool packed) {
    const int ntm = ceil_div(M, 256), ntn = ceil_div(N, 256);
    const char* e = getenv("PGK_GEMM256S");          // 0: two full stages, waves in lockstep; default: staggered phases
    if (!(packed || !e || atoi(e) != 0)) return G256_LOCKSTEP;
    const bool narrow = !accum_f32 && N % 192 == 0 && gemm256_narrow_fills_better(ntm, ntn, N / 192);      // 192-column tiles
    return narrow ? G256_STAGGERED_N192 : G256_STAGGERED;
}
// the SwiGLU epilogue: 128 act columns per tile, or 96 (192-column B tiles)
inline bool gemm256_swiglu_narrow(int M, int I) { return I % 96 == 0 && gemm256_narrow_fills_better(ceil_div(M, 256), I / 128, I / 96); }

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
