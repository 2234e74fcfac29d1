// Host-side kernel choice and grid size of the byte movers: the layout shuffles, gathers, KV-cache writes and argmax of
// ops_tensor.hip and the paged-cache / continuous-batching helpers of ops_paged.hip.  Every condition the launchers used to
// spell inline lives here as a pure function of the row's byte size, the item size and the OR of the addresses the launcher
// tests (only the low four bits count); the launchers call these functions and pgk_tensor_op_plan / pgk_tensor_op_grid
// (ops_tensor.hip) print the same return values, so the query cannot drift from the dispatch.  No device or stream is touched.
#pragma once

#include <cstddef>
#include <cstdint>
#include <initializer_list>

#include "pgk_internal.h"

namespace pgk {

constexpr int TN_BLOCK = 256;         // threads per block of every grid-stride mover
constexpr int TN_MAX_BLOCKS = 4096;   // the grid-stride kernels wrap beyond TN_MAX_BLOCKS * TN_BLOCK work items
constexpr int TN_TILE = 64;           // the LDS tile of transpose2d_kernel
constexpr int TN_MAX_BATCH = 65535;   // gridDim.z
constexpr int ARGMAX_WIDE_N = 16384;  // rows this long get 1024-thread blocks

// OR of the addresses a launcher tests: a vector width w fits when (bits % w) == 0
inline unsigned addr_bits(std::initializer_list<const void*> ptrs) {
    uintptr_t b = 0;
    for (const void* p : ptrs) b |= reinterpret_cast<uintptr_t>(p);
    return (unsigned)(b & 15u);
}

// the widest vector of 16, 8, 4, 2 or 1 bytes that divides row_bytes and keeps every tested pointer aligned
inline int pick_vec_bytes(size_t row_bytes, unsigned bits) {
    for (int w : {16, 8, 4, 2, 1})
        if (row_bytes % w == 0 && bits % w == 0) return w;
    return 1;
}

// split_qkv: as pick_vec_bytes over the three widths and four pointers, but never narrower than one element.  `bits` also
// carries the OR of the q, k and v row byte sizes: a power of two divides every one of them iff it divides their OR.
inline unsigned split_qkv_bits(size_t q_bytes, size_t k_bytes, size_t v_bytes, unsigned ptr_bits) {
    return (unsigned)((q_bytes | k_bytes | v_bytes | ptr_bits) & 15u);
}
inline int split_qkv_vec_bytes(int itemsize, unsigned bits) {
    int w = 16;
    for (; w > 1; w >>= 1) {
        if (w < itemsize) { w = itemsize; break; }
        if (bits % w == 0) break;
    }
    return w < itemsize ? itemsize : w;
}

// blocks of `block` threads over `items`, at least one, capped (the kernels grid-stride)
inline int cap_grid(size_t items, int block = TN_BLOCK) {
    size_t g = (items + block - 1) / block;
    if (g < 1) g = 1;
    return (int)(g > (size_t)TN_MAX_BLOCKS ? (size_t)TN_MAX_BLOCKS : g);
}

// pgk_paged_cache_write: a thread per 16-byte chunk of a (token, head) row; rows are whole chunks
inline bool paged_write_row_ok(size_t row_bytes) { return row_bytes % 16 == 0; }
inline int paged_write_grid(size_t rows, size_t row_bytes) { return cap_grid(rows * (row_bytes / 16)); }

// transpose2d_kernel: a block per 64 x 64 tile, the batch on gridDim.z
inline bool transpose_batch_ok(long long batch) { return batch >= 0 && batch <= TN_MAX_BATCH; }
inline int transpose_tiles_x(int cols) { return ceil_div(cols, TN_TILE); }
inline int transpose_tiles_y(int rows) { return ceil_div(rows, TN_TILE); }

// argmax_kernel: a block per row
inline int argmax_block(int n) { return n >= ARGMAX_WIDE_N ? 1024 : 256; }

inline const char* vec_leaf(int w) {
    switch (w) {
        case 16: return "vec16";
        case 8: return "vec8";
        case 4: return "vec4";
        case 2: return "vec2";
        default: return "vec1";
    }
}

}  // namespace pgk

// instantiate a kernel template on the vector type of `w` bytes
#define PGK_BY_VEC(w, ...)                                           \
    switch (w) {                                                     \
        case 16: { using V = uint4; __VA_ARGS__; } break;            \
        case 8: { using V = uint2; __VA_ARGS__; } break;             \
        case 4: { using V = uint32_t; __VA_ARGS__; } break;          \
        case 2: { using V = uint16_t; __VA_ARGS__; } break;          \
        default: { using V = uint8_t; __VA_ARGS__; } break;          \
    }
