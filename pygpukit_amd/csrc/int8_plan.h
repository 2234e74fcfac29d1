// Host-side kernel choice of the integer family (ops_int8.hip): pgk_gemm_int8_nt / pgk_gemm_int8_dequant_nt, pgk_gemm_int4_nt,
// pgk_gemv_int4 and pgk_linear_int8.  Pure functions of the shape, in the style of gemm_plan.h: the launchers switch on what
// these return and pgk_int_gemm_plan prints the same return values, so the query cannot drift from the dispatch.
#pragma once

#include <cstdlib>

#include "pgk_internal.h"

namespace pgk {

// ---- tile GEMMs on the i8 MFMA: 128 x 128 tiles, or 64 x 128 when those leave CUs idle ---------------------------------------
// A 64-row tile does half the work of a 128-row one and re-reads B twice as often, so it is only worth taking while the 128-row
// grid does not give every one of the 256 CUs a workgroup (or when there are no more than 64 rows at all).
enum IntGemmKernel { IG_SIMPLE = 0, IG_TILE128, IG_TILE64 };
constexpr int IG_FILL_WGS = 256;
inline IntGemmKernel int_tile_pick(int M, int N) {
    if (M <= 64) return IG_TILE64;
    return (long long)ceil_div(M, 128) * ceil_div(N, 128) < IG_FILL_WGS ? IG_TILE64 : IG_TILE128;
}
// int8: the fast path needs whole 16-byte chunks per row and aligned operands
inline IntGemmKernel gemm_int8_pick(int M, int N, int K, bool ptrs_aligned) {
    return K % 16 == 0 && ptrs_aligned ? int_tile_pick(M, N) : IG_SIMPLE;
}
// packed int4 (K/2 bytes per row): K % 32 == 0 and aligned operands
inline IntGemmKernel gemm_int4_pick(int M, int N, int K, bool ptrs_aligned) {
    return K % 32 == 0 && ptrs_aligned ? int_tile_pick(M, N) : IG_SIMPLE;
}
// The nibble-plane form multiplies 16 a by 16 b: it accumulates 256 x the sum, |16 a * 16 b| <= 2^14 per k, so the accumulator
// stays inside int32 while K * 2^14 <= 2^31 - 1.  Above that the tile kernel sign-extends the nibbles to int8 (4 ALU ops per
// plane where the shifted form takes 1 or 2) and accumulates the sum itself.
constexpr int INT4_PLANE_MAX_K = 131071;
inline bool gemm_int4_plane_form(int K) { return K <= INT4_PLANE_MAX_K; }

// ---- pgk_gemv_int4: rows per wave (a wave streams whole rows; more rows per wave when a row is short, so that a lane
// still has several 16-byte loads in flight) --------------------------------------------------------------------------------
enum Int4GemvKernel { I4V_SIMPLE = 0, I4V_STREAM };
inline Int4GemvKernel gemv_int4_pick(int K, bool ptrs_aligned) { return K % 32 == 0 && ptrs_aligned ? I4V_STREAM : I4V_SIMPLE; }
inline int gemv_int4_rows_per_wave(int K) { return K <= 2048 ? 4 : K <= 8192 ? 2 : 1; }   // <= 1 / <= 4 / more chunks per lane and row

// ---- pgk_linear_int8 (weight-only: 16-bit activations, int8 weights) ----------------------------------------------------------
// Few rows: every workgroup streams 16 weight rows once against the activations in LDS; more rows: the 16-bit MFMA tile
// loop with the weights converted on their way into LDS.
enum Lin8Kernel { L8_SIMPLE = 0, L8_STREAM, L8_MFMA };
constexpr int LIN8_STREAM_MAX_M = 8;
// PGK_LIN8_STREAM_MAX_M = 0..8 (read per call, as PGK_GEMM256 is) moves the switch down: tools/int8_bench.py times both leaves
// at the same row count with it.
inline int linear_int8_stream_max_m() {
    const char* e = getenv("PGK_LIN8_STREAM_MAX_M");
    const int v = e ? atoi(e) : LIN8_STREAM_MAX_M;
    return v < 0 ? 0 : v > LIN8_STREAM_MAX_M ? LIN8_STREAM_MAX_M : v;
}
inline Lin8Kernel linear_int8_pick(int M, int K, bool ptrs_aligned) {
    if (!(K % 16 == 0 && ptrs_aligned)) return L8_SIMPLE;
    return M <= linear_int8_stream_max_m() ? L8_STREAM : L8_MFMA;
}
inline int linear_int8_stream_mt(int M) { return M <= 1 ? 1 : M <= 2 ? 2 : M <= 4 ? 4 : 8; }   // rows held per lane (template)

}  // namespace pgk
