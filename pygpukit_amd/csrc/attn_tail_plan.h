// Request plan of the fused MFMA decode attention (attn_oproj_mfma_kernel, engine_attn.hip.h): which 16-row tiles a wave requests
// for a context of c1 cached rows, and how many of its requests are younger than the ones each counted wait is for.  Pure
// integer functions of (c1, chunk start, wave), used by the kernel itself and printed by pgk_attn_mfma_plan (the 192-row kernel)
// and pgk_attn_chunk_plan (any instantiated chunk length; both engine.hip) for the CPU tests that pin them.
//
// The chunk length CHUNK is a compile-time parameter of the kernel: T = CHUNK / 64 tiles per wave.  Per wave the vector memory
// requests are issued, and return, in this order:
//   issue phase:  NRAW new-token inputs | 4 T K of chunk 0 | 4 T V of chunk 0 | PRE W_o loads    (before the position is known)
//   later chunk:  4 n K | 4 n V                                                                  (n = am_live_tiles, 0 .. T)
// A tile is four requests of four rows per image.
#pragma once

namespace pgk {

constexpr int AM_CHUNK = 192;       // positions per staged chunk of the default kernel: 12 tiles, 3 per wave
constexpr int AM_CHUNK_WIDE = 256;  // ... of the single-pass kernel for 193..256 cached rows: 16 tiles, 4 per wave
constexpr int AM_WAVES = 4;
constexpr int AM_TILE_REQ = 4;      // requests per tile and image

constexpr bool am_chunk_valid(int chunk) { return chunk == AM_CHUNK || chunk == AM_CHUNK_WIDE; }
template <int CHUNK = AM_CHUNK>
__host__ __device__ constexpr int am_tiles_per_wave() { return CHUNK / (16 * AM_WAVES); }

// Wave w owns tiles w, w + 4, w + 8 (, w + 12) of a chunk: they ascend, so the live ones (first row below c1) are the first n.
template <int CHUNK = AM_CHUNK>
__host__ __device__ constexpr int am_live_tiles(int c0, int c1, int w) {
    constexpr int T = CHUNK / (16 * AM_WAVES);
    int n = 0;
    for (int u = 0; u < T; ++u) n += (c0 + 16 * (w + AM_WAVES * u) < c1) ? 1 : 0;
    return n;
}
// Row 4 q4 + r (lane quarter q4, score register r) of chunk tile `tile` counts: it is a cached row.  Every other staged row
// carries weight zero.
__host__ __device__ constexpr bool am_row_live(int c0, int c1, int tile, int q4, int r) { return c0 + 16 * tile + 4 * q4 + r < c1; }

// Counted waits ("at most this many outstanding").  Issue phase, pre = W_o preloads:
template <int CHUNK = AM_CHUNK>
__host__ __device__ constexpr int am_wait_new(int pre) { return 2 * am_tiles_per_wave<CHUNK>() * AM_TILE_REQ + pre; }   // younger than the new token's inputs: chunk 0 + W_o
template <int CHUNK = AM_CHUNK>
__host__ __device__ constexpr int am_wait_k0(int pre) { return am_tiles_per_wave<CHUNK>() * AM_TILE_REQ + pre; }        // ... than chunk 0's K: its V + W_o
__host__ __device__ constexpr int am_wait_v0(int pre) { return pre; }                          // ... than chunk 0's V: W_o
// later chunk with n live tiles: the V requests are younger than the K requests, nothing is younger than the V requests
__host__ __device__ constexpr int am_wait_k(int n) { return AM_TILE_REQ * n; }

// LDS of one workgroup of the kernel for a GQA group of G query heads: the two images, the waves' copies of the new token's
// inputs, the five state records, the normalised heads and the new token's q / k / v (the kernel asserts this sum against
// its own arrays).  A chunk length is instantiated for G only where this fits the CU's 160 KB.
constexpr int AM_LDS_CU = 160 * 1024;
constexpr int am_lds_bytes(int G, int chunk) {
    const int raw = ((G + 2) * 512 + 1024 + 1023) / 1024 * 1024;
    return 2 * chunk * 256 + AM_WAVES * raw + (AM_WAVES + 1) * G * (128 + 4) * 4 + G * 128 * 4 + (G + 2) * 256;
}
constexpr bool am_chunk_fits(int G, int chunk) { return am_chunk_valid(chunk) && am_lds_bytes(G, chunk) <= AM_LDS_CU; }

// The chunk length a fused single-sequence step with `rows` cached rows runs on: the wide kernel takes 193..256 rows in one
// pass where it fits; up to 192 rows are one pass of the default kernel already, and past 256 both walk two chunks, the
// default one with less LDS traffic per pass.
constexpr int am_pick_chunk(int G, int rows) {
    return (rows > AM_CHUNK && rows <= AM_CHUNK_WIDE && am_chunk_fits(G, AM_CHUNK_WIDE)) ? AM_CHUNK_WIDE : AM_CHUNK;
}

}  // namespace pgk
