// Request plan of the fused MFMA decode attention (attn_oproj_mfma_kernel, engine_attn.hip.h): which 16-row tiles a wave requests
// for a context of c1 cached rows, and how many of its requests are younger than the ones each counted wait is for.  Pure
// integer functions of (c1, chunk start, wave), used by the kernel itself and printed by pgk_attn_mfma_plan (engine.hip) for
// the CPU test that pins them.
//
// Per wave the vector memory requests are issued, and return, in this order:
//   issue phase:  NRAW new-token inputs | 12 K of chunk 0 | 12 V of chunk 0 | PRE W_o loads      (before the position is known)
//   later chunk:  4 n K | 4 n V                                                                  (n = am_live_tiles, 0 .. 3)
// A tile is four requests of four rows per image.
#pragma once

namespace pgk {

constexpr int AM_CHUNK = 192;   // positions per staged chunk: 12 tiles, 3 per wave
constexpr int AM_WAVES = 4;
constexpr int AM_TILE_REQ = 4;  // requests per tile and image

// Wave w owns tiles w, w + 4, w + 8 of a chunk: they ascend, so the live ones (first row below c1) are the first n.
__host__ __device__ constexpr int am_live_tiles(int c0, int c1, int w) {
    int n = 0;
    for (int u = 0; u < 3; ++u) n += (c0 + 16 * (w + AM_WAVES * u) < c1) ? 1 : 0;
    return n;
}

// Counted waits ("at most this many outstanding").  Issue phase, pre = W_o preloads:
__host__ __device__ constexpr int am_wait_new(int pre) { return 2 * 3 * AM_TILE_REQ + pre; }   // younger than the new token's inputs: chunk 0 + W_o
__host__ __device__ constexpr int am_wait_k0(int pre) { return 3 * AM_TILE_REQ + pre; }        // ... than chunk 0's K: its V + W_o
__host__ __device__ constexpr int am_wait_v0(int pre) { return pre; }                          // ... than chunk 0's V: W_o
// later chunk with n live tiles: the V requests are younger than the K requests, nothing is younger than the V requests
__host__ __device__ constexpr int am_wait_k(int n) { return AM_TILE_REQ * n; }

}  // namespace pgk
