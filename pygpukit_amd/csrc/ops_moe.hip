// Mixture-of-Experts routing and grouped expert GEMMs for gfx950 (reference: native/ops/moe/*.cuh and
// native/ops/matmul/gemm/w8a16_bf16/sm120/grouped_gemm.cu).
//
//   pgk_moe_topk_softmax        router logits [T,E] -> top-k weights (softmax over the k) + int32 expert ids; one wave per token
//   pgk_moe_compute_permutation stable counting sort of the T*k (token, slot) pairs by expert, plus the tile table
//   pgk_moe_gather / _scatter   rows into sorted order / weighted sum back per token (fp32, slot order, one rounding)
//   pgk_grouped_gemm_rows       C[r] = A[r] . W[e_r]^T for rows in any order (a plain fp32 kernel: not the hot path)
//   pgk_grouped_gemm_sorted     the same on rows grouped by expert, driven by the tile table:
//     few rows per expert (decode) - wsgemm_core.hip.h's walk (the one pgk_gemm_nt's skinny kernel runs) per (tile,
//       64-column slab, K split): the expert's rows sit in LDS, its weight streams from HBM straight into MFMA B
//       fragments, once per tile; split K writes fp32 slabs that the consumer (pgk_moe_scatter) sums in order;
//     many rows (prefill) - gemm_tile_core.hip.h's tile types and gemm_tile_loop.hip.h's 128 x 128 x 64 register-staged
//       loop (the ones gemm_mfma_kernel runs), each row tile inside one expert's segment and zero past its end.
//   Both kernels here add only the tile-table prologue, the a_map row gather and the r0-offset epilogue.
// No kernel here reads a device value back to the host: every grid is sized from T, k, E, N and K; workgroups whose tile
// table entry is empty exit at once.  No atomic decides an order, so two runs give identical bytes.

#include "gemm_plan.h"
#include "gemm_tile_core.hip.h"
#include "pgk_internal.h"
#include "wsgemm_core.hip.h"

namespace pgk {

constexpr int MOE_MAX_E = 256;
constexpr int MOE_MAX_K = 8;
constexpr int MOE_PERM_CHUNK = 4096;    // (token, slot) entries per permutation workgroup: 4 waves x 1024
// MOE_TILE_ROWS (rows per tile-table entry) and the regime / split / row-tile choices: gemm_plan.h

// softmax_topk_*_kernel (topk_kernels.cuh:192-260): max, exp(x - max) summed in order in fp32, times 1/sum
__device__ __forceinline__ void moe_softmax_k(float (&x)[MOE_MAX_K], int k) {
    float mx = x[0];
#pragma unroll
    for (int s = 1; s < MOE_MAX_K; ++s)
        if (s < k) mx = fmaxf(mx, x[s]);
    float sum = 0.f;
#pragma unroll
    for (int s = 0; s < MOE_MAX_K; ++s)
        if (s < k) { x[s] = expf(x[s] - mx); sum += x[s]; }
    const float inv = 1.0f / sum;
#pragma unroll
    for (int s = 0; s < MOE_MAX_K; ++s) x[s] *= inv;
}

// ------------------------------------------------------------------------------------------------ top-k + softmax ----
// One wave per token; lane l holds experts l, l+64, l+128, l+192.  k rounds of a wave arg-max whose order is (value
// descending, expert ascending): the reference's strict '>' scan (topk_kernels.cuh:49-64) keeps the lowest index among
// equal logits.  NaN logits compare as -inf.  Selected experts leave the race, so the k ids are distinct.
template <class T>
__global__ __launch_bounds__(256) void moe_topk_kernel(const T* logits, T* weights, int32_t* indices, int nT, int E, int k,
                                                       int do_softmax) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= nT) return;
    float v[4];
    bool live[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = lane + 64 * j;
        live[j] = e < E;
        const float x = live[j] ? to_f(logits[(size_t)t * E + e]) : -INFINITY;
        v[j] = x != x ? -INFINITY : x;
    }
    int sel_i[MOE_MAX_K];
#pragma unroll
    for (int s = 0; s < MOE_MAX_K; ++s) {
        sel_i[s] = 0;
        if (s < k) {
            float bv = -INFINITY;
            int bi = 0x7fffffff;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (live[j] && (v[j] > bv || bi == 0x7fffffff)) { bv = v[j]; bi = lane + 64 * j; }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const float ov = __shfl_xor(bv, off);
                const int oi = __shfl_xor(bi, off);
                if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
            }
            sel_i[s] = bi;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (bi == lane + 64 * j) live[j] = false;
        }
    }
    if (lane != 0) return;
    // the stored value is the logit as given (NaN included), as the reference stores local_logits[max_idx]
    float out[MOE_MAX_K];
#pragma unroll
    for (int s = 0; s < MOE_MAX_K; ++s) out[s] = s < k ? to_f(logits[(size_t)t * E + sel_i[s]]) : 0.f;
    if (do_softmax) moe_softmax_k(out, k);
#pragma unroll
    for (int s = 0; s < MOE_MAX_K; ++s)
        if (s < k) {
            weights[(size_t)t * k + s] = from_f<T>(out[s]);
            indices[(size_t)t * k + s] = sel_i[s];
        }
}

// in-place softmax over each row of k values (the reference's second routing step)
template <class T>
__global__ __launch_bounds__(256) void moe_softmax_k_kernel(T* w, int nT, int k) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nT) return;
    float x[MOE_MAX_K];
#pragma unroll
    for (int s = 0; s < MOE_MAX_K; ++s) x[s] = s < k ? to_f(w[(size_t)t * k + s]) : 0.f;
    moe_softmax_k(x, k);
#pragma unroll
    for (int s = 0; s < MOE_MAX_K; ++s)
        if (s < k) w[(size_t)t * k + s] = from_f<T>(x[s]);
}

// ------------------------------------------------------------------------------------------------ permutation ----
// Stable counting sort of the n = T*k flat entries (token-major, then slot) by expert, in three launches:
//   1. each wave counts its 1024 contiguous entries per expert  -> hist[wave slot][E]
//   2. one workgroup: per expert, exclusive prefix over wave slots; counts, offsets (exclusive scan over experts), the
//      tile table; hist becomes each wave slot's first output row per expert
//   3. each wave walks its entries in order, 64 at a time: an entry's rank among earlier lanes with the same expert comes
//      from 8 ballots (one per bit of the id), the last lane of each expert group advances the cursor.
// Expert ids outside [0, E) are not placed: their reverse_perm entry is -1 and the sorted rows end at offsets[E].
__device__ __forceinline__ bool moe_valid(int e, int E) { return e >= 0 && e < E; }

__global__ __launch_bounds__(256) void moe_hist_kernel(const int32_t* idx, int n, int E, int32_t* hist) {
    __shared__ int cnt[4][MOE_MAX_E];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int e = lane; e < E; e += 64) cnt[w][e] = 0;
    __syncthreads();
    const int base = blockIdx.x * MOE_PERM_CHUNK + w * (MOE_PERM_CHUNK / 4);
    for (int i = lane; i < MOE_PERM_CHUNK / 4; i += 64) {
        const int f = base + i;
        if (f >= n) break;
        const int e = idx[f];
        if (moe_valid(e, E)) atomicAdd(&cnt[w][e], 1);   // a count: its value does not depend on the order of the adds
    }
    __syncthreads();
    int32_t* h = hist + (size_t)(blockIdx.x * 4 + w) * E;
    for (int e = lane; e < E; e += 64) h[e] = cnt[w][e];
}

__global__ __launch_bounds__(256) void moe_offsets_kernel(int32_t* hist, int nslots, int E, int32_t* counts, int32_t* offsets,
                                                          int32_t* tiles, int max_tiles, int32_t* perm, int n) {
    __shared__ int scan[2][MOE_MAX_E];
    __shared__ int tscan[2][MOE_MAX_E];
    const int e = threadIdx.x;
    int total = 0;
    if (e < E)
        for (int s = 0; s < nslots; ++s) {
            const int c = hist[(size_t)s * E + e];
            hist[(size_t)s * E + e] = total;
            total += c;
        }
    const int ntile = (total + MOE_TILE_ROWS - 1) / MOE_TILE_ROWS;
    scan[0][e] = e < E ? total : 0;
    tscan[0][e] = e < E ? ntile : 0;
    __syncthreads();
    int p = 0;
    for (int off = 1; off < MOE_MAX_E; off <<= 1, p ^= 1) {   // inclusive Hillis-Steele scan over 256 slots
        scan[p ^ 1][e] = scan[p][e] + (e >= off ? scan[p][e - off] : 0);
        tscan[p ^ 1][e] = tscan[p][e] + (e >= off ? tscan[p][e - off] : 0);
        __syncthreads();
    }
    const int incl = scan[p][e], tincl = tscan[p][e];
    const int excl = incl - (e < E ? total : 0), texcl = tincl - (e < E ? ntile : 0);
    if (e < E) {
        counts[e] = total;
        offsets[e] = excl;
        if (e == E - 1) offsets[E] = incl;
        for (int s = 0; s < nslots; ++s) hist[(size_t)s * E + e] += excl;
        for (int j = 0; j < ntile; ++j) {
            tiles[2 * (texcl + j)] = e;
            tiles[2 * (texcl + j) + 1] = excl + j * MOE_TILE_ROWS;
        }
    }
    const int used = tscan[p][MOE_MAX_E - 1];
    for (int i = used + e; i < max_tiles; i += 256) {
        tiles[2 * i] = -1;
        tiles[2 * i + 1] = 0;
    }
    for (int i = scan[p][MOE_MAX_E - 1] + e; i < n; i += 256) perm[i] = -1;   // rows of entries with an invalid id
}

__global__ __launch_bounds__(256) void moe_place_kernel(const int32_t* idx, int n, int E, const int32_t* hist, int32_t* perm,
                                                        int32_t* rperm) {
    __shared__ int cur[4][MOE_MAX_E];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int32_t* h = hist + (size_t)(blockIdx.x * 4 + w) * E;
    for (int e = lane; e < E; e += 64) cur[w][e] = h[e];
    __syncthreads();
    const uint64_t lt = (1ull << lane) - 1ull;
    const int base = blockIdx.x * MOE_PERM_CHUNK + w * (MOE_PERM_CHUNK / 4);
    for (int i = 0; i < MOE_PERM_CHUNK / 4; i += 64) {
        const int f = base + i + lane;
        if (base + i >= n) break;                                  // wave-uniform
        const int e = f < n ? idx[f] : -1;
        const bool ok = f < n && moe_valid(e, E);
        uint64_t m = __ballot(ok);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const uint64_t bb = __ballot(ok && ((e >> b) & 1));
            m &= ((e >> b) & 1) ? bb : ~bb;
        }
        int pos = -1;
        if (ok) pos = cur[w][e] + __popcll(m & lt);
        __builtin_amdgcn_wave_barrier();                            // every lane has read its cursor before any update
        if (ok) {
            perm[pos] = f;
            if ((m >> lane) == 1ull) cur[w][e] += __popcll(m);      // the group's last lane
        }
        if (f < n) rperm[f] = pos;
        __builtin_amdgcn_wave_barrier();
    }
}

// ------------------------------------------------------------------------------------------------ gather / scatter ----
// gathered[r] = x[perm[r] / k]; rows whose perm entry is outside [0, n) (entries with an invalid id) are zero
__global__ __launch_bounds__(256) void moe_gather_kernel(const char* x, const int32_t* perm, int n, int k, int row_bytes, bool vec,
                                                         char* out) {
    const int r = blockIdx.x;
    const int f = perm[r];
    const bool ok = f >= 0 && f < n;
    const int src = ok ? f / k : 0;
    if (vec) {
        for (int c = threadIdx.x; c < row_bytes / 16; c += 256) {
            const uint4 v = ok ? *reinterpret_cast<const uint4*>(x + (size_t)src * row_bytes + 16 * c) : make_uint4(0, 0, 0, 0);
            *reinterpret_cast<uint4*>(out + (size_t)r * row_bytes + 16 * c) = v;
        }
    } else {
        for (int c = threadIdx.x; c < row_bytes / 2; c += 256) {
            const uint16_t v = ok ? reinterpret_cast<const uint16_t*>(x + (size_t)src * row_bytes)[c] : 0;
            reinterpret_cast<uint16_t*>(out + (size_t)r * row_bytes)[c] = v;
        }
    }
}

// out[t, h] = sum_slot w[t, slot] * y[rperm[t*k + slot], h], fp32 in slot order, one rounding (scatter_with_reverse_perm_kernel).
// y is either T [nrows][H] (splits == 0) or fp32 slabs [splits][nrows][H] summed in slab order first.
template <class T>
__global__ __launch_bounds__(256) void moe_scatter_kernel(const void* y, int splits, int nrows, const T* w, const int32_t* rperm,
                                                          T* out, int k, int H) {
    const int t = blockIdx.y;
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h >= H) return;
    float acc = 0.f;
    for (int s = 0; s < k; ++s) {
        const int r = rperm[(size_t)t * k + s];
        if (r < 0 || r >= nrows) continue;
        float v;
        if (splits == 0) {
            v = to_f(reinterpret_cast<const T*>(y)[(size_t)r * H + h]);
        } else {
            const float* ys = reinterpret_cast<const float*>(y);
            v = 0.f;
            for (int z = 0; z < splits; ++z) v += ys[((size_t)z * nrows + r) * H + h];
        }
        acc += to_f(w[(size_t)t * k + s]) * v;
    }
    out[(size_t)t * H + h] = from_f<T>(acc);
}

// row_expert_ids[r] = e with offsets[e] <= r < offsets[e+1]; -1 past offsets[E]
__global__ __launch_bounds__(256) void moe_expand_kernel(const int32_t* offsets, int E, int32_t* ids, int nrows) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= nrows) return;
    int lo = 0, hi = E;   // find the last e with offsets[e] <= r
    if (r >= offsets[E]) { ids[r] = -1; return; }
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= r) lo = mid; else hi = mid;
    }
    ids[r] = lo;
}

// ------------------------------------------------------------------------------------------------ grouped GEMM ----
// rows in any order: one workgroup per (row, 256 columns), one output per thread.  The weight is used as the reference
// uses it (grouped_gemm.cu:53-68): fp8 codes decoded and multiplied by the block scale in fp32, fp32 accumulation.
template <bool FP8>
__global__ __launch_bounds__(256) void grouped_rows_kernel(const bf16* A, const void* W, const bf16* ws, const int32_t* ids, bf16* C,
                                                           int M, int N, int K, int E) {
    const int r = blockIdx.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const int e = ids[r];
    float acc = 0.f;
    if (moe_valid(e, E)) {
        const bf16* a = A + (size_t)r * K;
        for (int k0 = 0; k0 < K; k0 += 8) {
            const uint4 av = *reinterpret_cast<const uint4*>(a + k0);
            float fa[8];
            WTraits<bf16>::decode(av, fa);
            float fw[8];
            if constexpr (FP8) {      // not fp8x8_to_bf16x8: the product stays fp32, it is never rounded to bf16
                const uint8_t* w = reinterpret_cast<const uint8_t*>(W) + ((size_t)e * N + n) * K + k0;
                const uint2 v = *reinterpret_cast<const uint2*>(w);
                const float sc = to_f(ws[((size_t)e * (N >> 7) + (n >> 7)) * (K >> 7) + (k0 >> 7)]);
                const f32x2 p0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.x, false), p1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.x, true);
                const f32x2 p2 = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.y, false), p3 = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.y, true);
                fw[0] = p0.x * sc; fw[1] = p0.y * sc; fw[2] = p1.x * sc; fw[3] = p1.y * sc;
                fw[4] = p2.x * sc; fw[5] = p2.y * sc; fw[6] = p3.x * sc; fw[7] = p3.y * sc;
            } else {
                WTraits<bf16>::decode(*reinterpret_cast<const uint4*>(reinterpret_cast<const bf16*>(W) + ((size_t)e * N + n) * K + k0), fw);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) acc += fa[j] * fw[j];
        }
    }
    C[(size_t)r * N + n] = from_f<bf16>(acc);
}

struct MoeGemmArgs {
    const bf16* a;          // [rows][K] sorted rows, or x [T][K] read through a_map
    const int32_t* a_map;   // NULL, or permute_indices: sorted row r reads x[a_map[r] / k]
    int k;
    const void* w;          // [E][N][K] bf16, or fp8 codes
    const bf16* wscale;     // fp8: [E][N/128][K/128]
    const int32_t* offsets; // [E+1]
    const int32_t* tiles;   // [max_tiles][2] = {expert or -1, first row}
    int N, K, nrows;        // nrows = T*k (C row count, slab stride)
    int k_per_split;
    void* c;                // splits == 0: bf16 [nrows][N]; else fp32 slabs [splits][nrows][N]
};

__device__ __forceinline__ int moe_src_row(const MoeGemmArgs& g, int r) { return g.a_map ? g.a_map[r] / g.k : r; }

// Weight-streaming regime: wsgemm_walk on one tile-table entry.  grid (N/64, splits, max_tiles); 4 waves x 16 weight rows;
// MT*16 >= the rows any tile can hold.
struct MoeWsProblem {
    const MoeGemmArgs& g;
    int r0;                 // first sorted row of the tile
    const void* w;          // the expert's weight and scales
    const bf16* wscale;
    int M, N, K, kbeg, kend;
    __device__ __forceinline__ const bf16* a_row(int r) const { return g.a + (size_t)moe_src_row(g, r0 + min(r, M - 1)) * K; }
};

template <int MT, bool FP8, bool SLAB>
__global__ __launch_bounds__(WS_THREADS) void moe_ws_kernel(MoeGemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char a_lds[];
    const int e = load_uniform_i32(g.tiles + 2 * blockIdx.z);
    if (e < 0) return;
    const int r0 = load_uniform_i32(g.tiles + 2 * blockIdx.z + 1);
    const int M = min(min(load_uniform_i32(g.offsets + e + 1) - r0, MOE_TILE_ROWS), MT * 16);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int n0 = (blockIdx.x * 4 + wid) * 16;
    const int kbeg = blockIdx.y * g.k_per_split;
    const MoeWsProblem p{g, r0, reinterpret_cast<const char*>(g.w) + (size_t)e * g.N * g.K * (FP8 ? 1 : 2),
                         FP8 ? g.wscale + (size_t)e * (g.N >> 7) * (g.K >> 7) : nullptr,
                         M, g.N, g.K, kbeg, min(kbeg + g.k_per_split, g.K)};

    f32x4_t acc[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) acc[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // row tiles past M are neither read nor multiplied; each A fragment is read right before its MFMA, not one k-step ahead:
    // reading ahead takes MT*8 more registers, which in this kernel (it holds r0 and the expert's bases besides) costs a wave
    // of occupancy at MT = 2 (4 -> 3) and at MT = 4 fp8 (3 -> 2)
    wsgemm_walk<MT, FP8, true, false>(p, a_lds, n0, acc);

    const int n = n0 + (lane & 15);
    if (n >= g.N) return;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = mt * 16 + (lane >> 4) * 4 + r;
            if (m >= M) continue;
            const size_t row = (size_t)(r0 + m);
            if constexpr (SLAB) reinterpret_cast<float*>(g.c)[((size_t)blockIdx.y * g.nrows + row) * g.N + n] = acc[mt][r];
            else reinterpret_cast<bf16*>(g.c)[row * g.N + n] = from_f<bf16>(acc[mt][r]);
        }
}

// Tiled regime: the gemm_tile_loop.hip.h loop on one tile-table entry and 128 columns: A rows gathered through a_map (rows past the
// expert's segment are zero), B the expert's weight.  grid (max_tiles, N/128).
template <bool FP8, bool SLAB>
__global__ __launch_bounds__(GEMM_THREADS) void moe_tile_kernel(MoeGemmArgs g) {
    constexpr int BM = 128, BN = 128;
    __shared__ __attribute__((aligned(16))) char smem[gemm_tile_lds_bytes(BM, BN)];
    const int e = load_uniform_i32(g.tiles + 2 * blockIdx.x);
    if (e < 0) return;
    const int r0 = load_uniform_i32(g.tiles + 2 * blockIdx.x + 1);
    const int M = min(load_uniform_i32(g.offsets + e + 1) - r0, BM);
    const int K = g.K, N = g.N;
    const int n0 = blockIdx.y * BN;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    const char* wbase = reinterpret_cast<const char*>(g.w) + (size_t)e * N * K * (FP8 ? 1 : 2);
    const bf16* sbase = FP8 ? g.wscale + (size_t)e * (N >> 7) * (K >> 7) : nullptr;

    TileRegsK<BM> ra;
    TileRegsK<BN> rb;
    TileRegsFp8NT<BN> rb_f8;
    const bf16* arow[TileRegsK<BM>::CH];      // rows past M read a clamped row and are stored as zeros
    bool aok[TileRegsK<BM>::CH];
#pragma unroll
    for (int i = 0; i < TileRegsK<BM>::CH; ++i) {
        const int r = (threadIdx.x + i * GEMM_THREADS) >> 3;
        aok[i] = r < M;
        arow[i] = g.a + (size_t)moe_src_row(g, r0 + min(r, M - 1)) * K;
    }
    auto load_tiles = [&](int k0) {
        ra.load_rows(arow, k0, K);
        if constexpr (FP8) rb_f8.load(reinterpret_cast<const uint8_t*>(wbase), sbase, n0, N, k0, K);
        else rb.load(reinterpret_cast<const bf16*>(wbase), n0, N, k0, K, K);
    };
    auto store_tiles = [&](int buf) {
        char* as = gemm_tile_a<BM, BN>(smem, buf);
        char* bs = gemm_tile_b<BM, BN>(smem, buf);
        ra.store_rows(as, aok);
        if constexpr (FP8) rb_f8.store(bs);
        else rb.store(bs);
    };

    f32x4_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    using T = bf16;
    const int kbeg = 0, kend = K;
#include "gemm_tile_loop.hip.h"      // the main loop: acc += A . B^T over [kbeg, kend)

#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = n0 + wn * 64 + j * 16 + (lane & 15);
            if (col >= N) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = wm * 64 + i * 16 + (lane >> 4) * 4 + r;
                if (m >= M) continue;
                const size_t row = (size_t)(r0 + m);
                if constexpr (SLAB) reinterpret_cast<float*>(g.c)[row * N + col] = acc[i][j][r];
                else reinterpret_cast<bf16*>(g.c)[row * N + col] = from_f<bf16>(acc[i][j][r]);
            }
        }
}

// MT x FP8 x SLAB -> the instantiation (its LDS limit raised once where MT*16 rows of 512 bytes pass 48 KiB)
template <int MT, bool FP8>
static pgk_status moe_ws_launch_slab(const MoeGemmArgs& g, bool slab, dim3 grid, hipStream_t st) {
    constexpr size_t lds = ws_lds_bytes(MT);
    constexpr bool raise = lds > 48 * 1024;
    if (slab) return launch_dyn_lds<&moe_ws_kernel<MT, FP8, true>>(grid, WS_THREADS, lds, raise, st, g);
    return launch_dyn_lds<&moe_ws_kernel<MT, FP8, false>>(grid, WS_THREADS, lds, raise, st, g);
}
template <int MT>
static pgk_status moe_ws_launch(const MoeGemmArgs& g, bool fp8, bool slab, dim3 grid, hipStream_t st) {
    return fp8 ? moe_ws_launch_slab<MT, true>(g, slab, grid, st) : moe_ws_launch_slab<MT, false>(g, slab, grid, st);
}

}  // namespace pgk

using namespace pgk;

extern "C" {

pgk_status pgk_moe_topk_softmax(const void* logits, void* weights, int32_t* indices, int T, int E, int k, int softmax,
                                pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(logits && weights && indices, "pgk_moe_topk_softmax: null pointer");
    PGK_REQUIRE(T >= 0 && E >= 1 && E <= MOE_MAX_E, "pgk_moe_topk_softmax: num_experts=%d outside [1, %d]", E, MOE_MAX_E);
    PGK_REQUIRE(k >= 1 && k <= MOE_MAX_K && k <= E, "pgk_moe_topk_softmax: k=%d outside [1, min(%d, num_experts=%d)]", k, MOE_MAX_K, E);
    PGK_REQUIRE(dt == PGK_BF16 || dt == PGK_F32, "pgk_moe_topk_softmax: logits must be bf16 or fp32 (dtype %d)", (int)dt);
    if (!T) return PGK_OK;
    hipStream_t st = resolve_stream(s);
    if (dt == PGK_BF16)
        moe_topk_kernel<bf16><<<ceil_div(T, 4), 256, 0, st>>>((const bf16*)logits, (bf16*)weights, indices, T, E, k, softmax ? 1 : 0);
    else
        moe_topk_kernel<float><<<ceil_div(T, 4), 256, 0, st>>>((const float*)logits, (float*)weights, indices, T, E, k, softmax ? 1 : 0);
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

pgk_status pgk_moe_softmax_topk(void* weights, int T, int k, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(weights, "pgk_moe_softmax_topk: null pointer");
    PGK_REQUIRE(T >= 0 && k >= 1 && k <= MOE_MAX_K, "pgk_moe_softmax_topk: k=%d outside [1, %d]", k, MOE_MAX_K);
    PGK_REQUIRE(dt == PGK_BF16 || dt == PGK_F32, "pgk_moe_softmax_topk: values must be bf16 or fp32 (dtype %d)", (int)dt);
    if (!T) return PGK_OK;
    hipStream_t st = resolve_stream(s);
    if (dt == PGK_BF16) moe_softmax_k_kernel<bf16><<<ceil_div(T, 256), 256, 0, st>>>((bf16*)weights, T, k);
    else moe_softmax_k_kernel<float><<<ceil_div(T, 256), 256, 0, st>>>((float*)weights, T, k);
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

int pgk_moe_max_tiles(int T, int k, int E) { return moe_max_tiles(T, k, E); }

size_t pgk_moe_workspace_bytes(int T, int k, int E) {
    return (size_t)ceil_div((long long)T * k, MOE_PERM_CHUNK) * 4 * (size_t)E * sizeof(int32_t);
}

pgk_status pgk_moe_compute_permutation(const int32_t* indices, int T, int k, int E, int32_t* counts, int32_t* offsets,
                                       int32_t* permute_indices, int32_t* reverse_perm, int32_t* tiles, void* workspace,
                                       pgk_stream s) {
    PGK_REQUIRE(indices && counts && offsets && permute_indices && reverse_perm && tiles, "pgk_moe_compute_permutation: null pointer");
    PGK_REQUIRE(T >= 0 && k >= 1 && E >= 1 && E <= MOE_MAX_E, "pgk_moe_compute_permutation: bad shape T=%d k=%d E=%d", T, k, E);
    PGK_REQUIRE((long long)T * k < (1ll << 30), "pgk_moe_compute_permutation: T*k=%lld too large", (long long)T * k);
    const int n = T * k;
    const int nb = ceil_div(n, MOE_PERM_CHUNK);
    PGK_REQUIRE(n == 0 || workspace, "pgk_moe_compute_permutation: null workspace");
    hipStream_t st = resolve_stream(s);
    int32_t* hist = (int32_t*)workspace;
    if (nb) moe_hist_kernel<<<nb, 256, 0, st>>>(indices, n, E, hist);
    moe_offsets_kernel<<<1, 256, 0, st>>>(hist, nb * 4, E, counts, offsets, tiles, moe_max_tiles(T, k, E), permute_indices, n);
    if (nb) moe_place_kernel<<<nb, 256, 0, st>>>(indices, n, E, hist, permute_indices, reverse_perm);
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

pgk_status pgk_moe_gather(const void* x, const int32_t* permute_indices, void* gathered, int T, int k, int H, pgk_dtype dt,
                          pgk_stream s) {
    PGK_REQUIRE(x && permute_indices && gathered, "pgk_moe_gather: null pointer");
    PGK_REQUIRE(T >= 0 && k >= 1 && H >= 1, "pgk_moe_gather: bad shape T=%d k=%d H=%d", T, k, H);
    PGK_REQUIRE(dt == PGK_BF16 || dt == PGK_F16 || dt == PGK_F32, "pgk_moe_gather: unsupported dtype %d", (int)dt);
    if (!T) return PGK_OK;
    const int row_bytes = H * (int)dtype_size(dt);
    const bool vec = row_bytes % 16 == 0 && aligned16(x) && aligned16(gathered);
    moe_gather_kernel<<<T * k, 256, 0, resolve_stream(s)>>>((const char*)x, permute_indices, T * k, k, row_bytes, vec, (char*)gathered);
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

pgk_status pgk_moe_scatter(const void* y, int splits, const void* weights, const int32_t* reverse_perm, void* out, int nT, int k,
                           int H, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(y && weights && reverse_perm && out, "pgk_moe_scatter: null pointer");
    PGK_REQUIRE(nT >= 0 && k >= 1 && H >= 1 && splits >= 0 && splits <= 64, "pgk_moe_scatter: bad shape T=%d k=%d H=%d splits=%d", nT, k, H, splits);
    if (!nT) return PGK_OK;
    dim3 grid(ceil_div(H, 256), nT);
    hipStream_t st = resolve_stream(s);
    PGK_DISPATCH_FLOAT(dt, "pgk_moe_scatter",
                       (moe_scatter_kernel<T><<<grid, 256, 0, st>>>(y, splits, nT * k, (const T*)weights, reverse_perm, (T*)out, k, H)));
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

pgk_status pgk_moe_expand_expert_offsets(const int32_t* offsets, int E, int32_t* row_expert_ids, int nrows, pgk_stream s) {
    PGK_REQUIRE(offsets && row_expert_ids, "pgk_moe_expand_expert_offsets: null pointer");
    PGK_REQUIRE(E >= 1 && nrows >= 0, "pgk_moe_expand_expert_offsets: bad shape E=%d rows=%d", E, nrows);
    if (!nrows) return PGK_OK;
    moe_expand_kernel<<<ceil_div(nrows, 256), 256, 0, resolve_stream(s)>>>(offsets, E, row_expert_ids, nrows);
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

static pgk_status grouped_check(const char* name, const void* a, const void* w, const void* wscale, int fp8, void* c, int N, int K, int E) {
    PGK_REQUIRE(a && w && c && (!fp8 || wscale), "%s: null pointer", name);
    PGK_REQUIRE(N >= 1 && K >= 8 && E >= 1, "%s: bad shape N=%d K=%d E=%d", name, N, K, E);
    if (fp8) PGK_REQUIRE(K % 128 == 0 && N % 128 == 0, "%s: fp8 weights need K=%d and N=%d to be multiples of the 128x128 scale block", name, K, N);
    else PGK_REQUIRE(K % 8 == 0 && N % 8 == 0, "%s: bf16 weights need K=%d and N=%d to be multiples of 8", name, K, N);
    PGK_REQUIRE(aligned16(a) && aligned16(w) && aligned16(c), "%s: operands must be 16-byte aligned", name);
    return PGK_OK;
}

pgk_status pgk_grouped_gemm_rows(const void* a, const void* w, const void* wscale, int fp8, void* c, const int32_t* row_expert_ids,
                                 int M, int N, int K, int E, pgk_stream s) {
    if (pgk_status r = grouped_check("pgk_grouped_gemm_rows", a, w, wscale, fp8, c, N, K, E)) return r;
    PGK_REQUIRE(row_expert_ids && M >= 0, "pgk_grouped_gemm_rows: bad row ids / M=%d", M);
    if (!M) return PGK_OK;
    dim3 grid(ceil_div(N, 256), M);
    hipStream_t st = resolve_stream(s);
    if (fp8) grouped_rows_kernel<true><<<grid, 256, 0, st>>>((const bf16*)a, w, (const bf16*)wscale, row_expert_ids, (bf16*)c, M, N, K, E);
    else grouped_rows_kernel<false><<<grid, 256, 0, st>>>((const bf16*)a, w, nullptr, row_expert_ids, (bf16*)c, M, N, K, E);
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

int pgk_grouped_gemm_sorted_splits(int T, int k, int E, int N, int K) {
    if (T < 1 || k < 1 || E < 1 || N < 1 || K < 8) return 1;
    return moe_sorted_splits(T, k, E, N, K);
}

pgk_status pgk_grouped_gemm_sorted(const void* a, const int32_t* a_map, const void* w, const void* wscale, int fp8, void* c,
                                   int splits, const int32_t* offsets, const int32_t* tiles, int T, int k, int E, int N, int K,
                                   pgk_stream s) {
    if (pgk_status r = grouped_check("pgk_grouped_gemm_sorted", a, w, wscale, fp8, c, N, K, E)) return r;
    PGK_REQUIRE(offsets && tiles && T >= 0 && k >= 1 && E <= MOE_MAX_E, "pgk_grouped_gemm_sorted: bad routing arguments T=%d k=%d E=%d", T, k, E);
    PGK_REQUIRE((long long)T * k < (1ll << 30), "pgk_grouped_gemm_sorted: T*k too large");
    if (!T) return PGK_OK;
    const int want = moe_sorted_splits(T, k, E, N, K);
    PGK_REQUIRE(splits == 0 || splits == want, "pgk_grouped_gemm_sorted: splits=%d, this shape takes 0 (bf16 C) or %d (fp32 slabs)", splits, want);
    MoeGemmArgs g{(const bf16*)a, a_map, k, w, (const bf16*)wscale, offsets, tiles, N, K, T * k, 0, c};
    const int tiles_n = moe_max_tiles(T, k, E);
    hipStream_t st = resolve_stream(s);
    const bool slab = splits > 0;
    if (!moe_ws_regime(T, k, E)) {
        dim3 grid(tiles_n, ceil_div(N, 128));
#define PGK_MOE_TILE(F8, SL) moe_tile_kernel<F8, SL><<<grid, 256, 0, st>>>(g)
        if (fp8) { if (slab) PGK_MOE_TILE(true, true); else PGK_MOE_TILE(true, false); }
        else { if (slab) PGK_MOE_TILE(false, true); else PGK_MOE_TILE(false, false); }
#undef PGK_MOE_TILE
        PGK_LAUNCH_CHECK();
        return PGK_OK;
    }
    const int nsplit = slab ? splits : 1;
    g.k_per_split = ceil_div(ceil_div(K, nsplit), WS_KT) * WS_KT;
    dim3 grid(ceil_div(N, 64), nsplit, tiles_n);
    switch (moe_ws_pick_mt(T, k)) {      // gemm_plan.h: 1, 2, 4 or 8 tiles of 16 rows
        case 1: return moe_ws_launch<1>(g, fp8 != 0, slab, grid, st);
        case 2: return moe_ws_launch<2>(g, fp8 != 0, slab, grid, st);
        case 4: return moe_ws_launch<4>(g, fp8 != 0, slab, grid, st);
        case 8: return moe_ws_launch<8>(g, fp8 != 0, slab, grid, st);
    }
    return set_error(PGK_ERR_INVALID, "pgk_grouped_gemm_sorted: no tile for T*k=%d rows", T * k);
}

}  // extern "C"
