// Host-side kernel choice and grid size of the base ops: the elementwise family (ops_elementwise.hip), the row norms and RoPE
// (ops_norm_rope.hip), clamp / where (ops_reduce.hip).  Every condition the launchers used to spell inline lives here as a pure
// function of the element count or row shape, the item size and "every pointer the launcher tests is 16-byte aligned"; the
// launchers call these functions and pgk_base_op_plan / pgk_base_op_grid (ops_elementwise.hip) print the same return values, so
// the query cannot drift from the dispatch.  No device, stream or pointer is touched here.
#pragma once

#include <cstddef>

#include "pgk_internal.h"

namespace pgk {

constexpr int EW_BLOCK = 256;
constexpr int EW_MAX_BLOCKS = 2048;
constexpr int RD_BLOCK = 256;
constexpr int RD_MAX_BLOCKS = 1024;
constexpr int NORM_WAVES = 4;  // rows per block in the wave-per-row kernels
constexpr int NORM_MAXV = 8;   // 16-byte vectors per lane held in registers

inline int vec_elems(size_t item) { return (int)(16 / item); }   // Vec<T>::N

// blocks of EW_BLOCK threads over `work_items`, at least one, capped (the kernels grid-stride)
inline int ew_grid(size_t work_items) {
    size_t g = (work_items + EW_BLOCK - 1) / EW_BLOCK;
    if (g < 1) g = 1;
    return (int)(g > EW_MAX_BLOCKS ? EW_MAX_BLOCKS : g);
}

// ---- pgk_binary, pgk_activation, pgk_glu: 16-byte accesses plus a scalar tail, or scalar accesses throughout ------------------
enum EwKernel { EW_VEC = 0, EW_SCALAR = 1 };
inline EwKernel ew_flat_pick(bool ptrs_aligned) { return ptrs_aligned ? EW_VEC : EW_SCALAR; }
// a thread per vector (n / N of them, + 1 so that the tail has a thread when n < N), or a thread per element
inline int ew_flat_grid(size_t n, size_t item, bool ptrs_aligned) {
    return ew_grid(ew_flat_pick(ptrs_aligned) == EW_VEC ? n / vec_elems(item) + 1 : n);
}

// ---- pgk_bias_add_inplace, pgk_glu_packed: whole vectors per row (features % N == 0), or scalar --------------------------------
enum RowKernel { ROW_VEC = 0, ROW_SCALAR = 1 };
inline RowKernel ew_row_pick(int features, size_t item, bool ptrs_aligned) {
    return ptrs_aligned && (features % vec_elems(item) == 0) ? ROW_VEC : ROW_SCALAR;
}
inline int ew_row_grid(size_t rows, int features, size_t item, bool ptrs_aligned) {
    const size_t n = rows * (size_t)features;
    return ew_grid(ew_row_pick(features, item, ptrs_aligned) == ROW_VEC ? n / vec_elems(item) : n);
}

// ---- pgk_cast: one kernel, 4 elements per thread per trip plus a scalar tail ---------------------------------------------------
inline int cast_grid(size_t n) { return ew_grid(n / 4 + 1); }

// ---- launch_norm: a wave per row with the row in registers, or a 256-thread block per row with scalar accesses -----------------
enum NormKernel { NORM_WAVE = 0, NORM_BLOCK = 1 };
// ptrs_aligned: x, out, gamma, and residual (rmsnorm_residual) / beta (layernorm)
inline NormKernel norm_pick(int features, size_t item, bool ptrs_aligned) {
    const int N = vec_elems(item);
    return (features % N == 0) && features <= 64 * N * NORM_MAXV && ptrs_aligned && ((size_t)features * item) % 16 == 0
               ? NORM_WAVE : NORM_BLOCK;
}
inline int norm_grid(int rows, int features, size_t item, bool ptrs_aligned) {
    return norm_pick(features, item, ptrs_aligned) == NORM_WAVE ? ceil_div(rows, NORM_WAVES) : rows;
}

// ---- pgk_adaln_fused (ops_diffusion.hip): the same two kernels, rows of [batch, tokens, features] ------------------------------
// ptrs_aligned: x, residual, sum_out, y, every table and vector that is given, and every vector's batch stride in bytes
inline NormKernel adaln_pick(int features, size_t item, bool ptrs_aligned) { return norm_pick(features, item, ptrs_aligned); }
inline const char* adaln_leaf(int features, size_t item, bool ptrs_aligned) {
    return adaln_pick(features, item, ptrs_aligned) == NORM_WAVE ? "adaln_wave" : "adaln_block";
}

// ---- pgk_rope_inplace: a thread per (x[d], x[d + D/2]) pair, 256 per block ------------------------------------------------------
inline int rope_grid(size_t pairs) { return (int)((pairs + 255) / 256 > 2048 ? 2048 : (pairs + 255) / 256); }

// ---- pgk_clamp, pgk_where, pgk_reduce (first level), pgk_widen_i32_i64: a thread per element ------------------------------------
inline int rd_grid(size_t n) {
    const size_t g = (n + RD_BLOCK - 1) / RD_BLOCK;
    return (int)(g < 1 ? 1 : (g > RD_MAX_BLOCKS ? RD_MAX_BLOCKS : g));
}

}  // namespace pgk
