// Batched multi-head latent attention decode over a PAGED latent cache [num_blocks][block_size][576]: a page row is a row of the
// contiguous cache of ops_mla.hip, [c (512) | kpe (64)], one per token for all heads, so the pages have no head axis.
//   pgk_mla_paged_cache_write   kv_a [n][576] -> slot slot_mapping[t]: rmsnorm of the first 512 columns, RoPE of the last 64 at
//                               positions[t]; mla_cache_write_kernel's expressions in its order, so the bits of a slot are those of
//                               row positions[t] of a contiguous cache
//   pgk_sdpa_mla_paged          out[b][i][h] = sum_r softmax_r(scale <q[b][i][h], row_b(r)>) row_b(r)[:512], r <= context_lens[b] - q_len + i,
//                               row_b(r) = page block_tables[b][r / block_size], row r % block_size
//
// mla_paged_kernel: grid (column tiles, KV chunks, sequences), 4 waves.  The tile walk is mla_decode_kernel's, line for line - the
// padded row-major image of 32 latent rows, S^T = C . Q^T split over the contraction with the four partial tiles summed out of LDS, the
// redundant fp32 exp2 softmax, O^T += C^T . P^T through ds_read_b64_tr_b16, the (m ln 2, l, O[512]) record - as a second kernel, not a
// shared core: the fixed-cache kernel's code object stays what it was.  What is new is where a tile's rows come from:
//   * the chunk count is mla_paged_chunks(H, q_len, num_seqs, max_context), a host function of the shape alone, so the grid and the
//     workspace never depend on device data; the LIVE chunk length is decode_chunk_len of the sequence's own context_lens[b], read
//     here.  A workgroup whose chunk is empty for its sequence (a short or idle sequence in a batch sized by a long one) loads no
//     query, resolves no row, reads no page and leaves the neutral record (-inf, 0, 0) - or zeros in `out` with one chunk;
//   * a thread's 9 sixteen-byte pieces of a tile fall in up to 9 different rows, so the block table is NOT consulted per piece: the 32
//     lanes of the first half-wave resolve the 32 physical row numbers of tile t + 2 (one division, one table entry each) while the
//     MFMAs of tile t run, and park them in a double-buffered LDS array after the trip's second barrier; tile t + 1's loads are issued
//     at the top of the trip from the array filled a trip earlier.  No table load ever sits between a barrier and the page loads
//     that need it: those read LDS.  (The alternative, every thread resolving its own rows, is 9 divisions and 9 dependent table
//     loads per thread and tile in front of the loads the walk waits for.)
//   * a row at or beyond the chunk's live end (never past the context) resolves to -1 without touching the table: its image row is
//     zero and its score masked, as in the fixed-cache kernel, so no table entry at or beyond ceil(context / block_size) is ever
//     dereferenced, the look-ahead included, and no byte of a page row at or beyond the context enters a product.  An entry outside
//     the page pool also resolves to -1 (a zero row) instead of an address.
// Resources: the fixed-cache kernel's plus 256 bytes of LDS for the row numbers (profiles/mla_paged_isa.txt).

#include "attn_core.hip.h"
#include "flash_common.hip.h"
#include "pgk_internal.h"

namespace pgk {

constexpr int MLA_ROWB = MLA_WIDTH * 2 + 16;                 // bytes per image row (ops_mla.hip)
constexpr int MLA_IMG = MLA_KEYS * MLA_ROWB;
constexpr int MLA_RED = 4 * 16 * 64 * 4;                     // partial scores: [wave][register][lane] fp32
constexpr int MLA_MAP = 2 * MLA_KEYS * 4;                    // physical row numbers of two tiles
constexpr int MLA_PAGED_LDS = MLA_IMG + MLA_RED + MLA_MAP;
constexpr int MLA_STAGE = MLA_KEYS * (MLA_WIDTH / 8) / 256;  // 16-byte pieces a thread stages per tile
constexpr int MLA_KS = MLA_WIDTH / 4 / 16;                   // k-steps of a wave's quarter of the contraction
constexpr int MLA_REC = MLA_LATENT + 2;
static_assert(MLA_STAGE * 256 == MLA_KEYS * (MLA_WIDTH / 8) && MLA_KS * 64 == MLA_WIDTH && MLA_COLS == 32 && MLA_KEYS == 32, "mla tile");

typedef short mla_v4s __attribute__((ext_vector_type(4)));

template <class T>
__global__ __launch_bounds__(256, 2) void mla_paged_kernel(const T* q, const T* cache, const int32_t* block_tables, const int32_t* context_lens,
                                                        T* out, float* ws, int heads, int q_len, int block_size, int max_blocks, int num_blocks,
                                                        int max_context, int nchunks, float scale_log2e) {
    extern __shared__ __attribute__((aligned(16))) char mla_smem[];      // image | partial scores | row numbers
    char* img = mla_smem;
    float* red = reinterpret_cast<float*>(mla_smem + MLA_IMG);
    int* rowmap = reinterpret_cast<int*>(mla_smem + MLA_IMG + MLA_RED);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, ql = lane & 31, hh = lane >> 5;
    const int b = blockIdx.z, ncols = heads * q_len, col0 = blockIdx.x * MLA_COLS, col = col0 + ql;
    // the sequence's own length: clamped to the bound the grid was sized by and to the table; 0 < ctx < q_len is idle
    int ctx = min(context_lens[b], (int)min((long long)max_context, (long long)max_blocks * block_size));
    if (ctx < q_len) ctx = 0;
    const bool live = col < ncols;                           // a tail column: zero query, never stored
    const int moff = ctx - q_len;                            // query row i sees keys <= moff + i
    const int lim = moff + min(col, ncols - 1) / heads;
    const int kv_end = ctx > 0 ? moff + min(col0 + MLA_COLS - 1, ncols - 1) / heads + 1 : 0;      // keys the tile's last live column sees (<= ctx)
    const int clen = decode_chunk_len(ctx, nchunks, MLA_KEYS);
    const int c0 = min((int)blockIdx.y * clen, kv_end), c1 = min(c0 + clen, kv_end);
    const int nt = (c1 - c0 + MLA_KEYS - 1) / MLA_KEYS;      // 0: this chunk is empty for this sequence
    const int limc = min(lim, c1 - 1);
    const int32_t* tbl = block_tables + (size_t)b * max_blocks;

    // Q^T fragments (B operand): lane = column, k = depth 144 wid + 16 ks + 8 hh .. + 7, the caller's bits
    uint4 qf[MLA_KS];
    {
        const T* qrow = q + ((size_t)b * ncols + min(col, ncols - 1)) * MLA_WIDTH + wid * (MLA_WIDTH / 4) + 8 * hh;
#pragma unroll
        for (int ks = 0; ks < MLA_KS; ++ks) qf[ks] = live && nt > 0 ? *reinterpret_cast<const uint4*>(qrow + ks * 16) : make_uint4(0, 0, 0, 0);
    }
    f32x16_fl o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    // ---- the paged issue stage --------------------------------------------------------------------------------------------------
    // physical row of the chunk's row 32 t + tid (tid < 32): -1 at or beyond c1 WITHOUT a table access, and for an entry outside the pool
    auto resolve = [&](int t) -> int {
        const int row = c0 + t * MLA_KEYS + tid;
        if (row >= c1) return -1;
        const int blk = row / block_size;
        const int e = tbl[blk];
        return (unsigned)e < (unsigned)num_blocks ? e * block_size + (row - blk * block_size) : -1;
    };
    // piece tid + 256 j of the tile's 2304, row (tid + 256 j) / 72, from the row numbers resolved a trip earlier; zero for row -1
    uint4 st[MLA_STAGE];
    auto load_tile = [&](int t) {
        const int* rm = rowmap + (t & 1) * MLA_KEYS;
#pragma unroll
        for (int j = 0; j < MLA_STAGE; ++j) {
            const int c = tid + 256 * j, r = c / (MLA_WIDTH / 8), cc = c % (MLA_WIDTH / 8);
            const int pr = rm[r];
            st[j] = make_uint4(0, 0, 0, 0);
            if (pr >= 0) st[j] = *reinterpret_cast<const uint4*>(cache + (size_t)pr * MLA_WIDTH + cc * 8);
        }
    };
    auto store_tile = [&] {
#pragma unroll
        for (int j = 0; j < MLA_STAGE; ++j) {
            const int c = tid + 256 * j, r = c / (MLA_WIDTH / 8), cc = c % (MLA_WIDTH / 8);
            *reinterpret_cast<uint4*>(img + r * MLA_ROWB + cc * 16) = st[j];
        }
    };
    // C^T fragment of (k-step s, half u, latent tile i of this wave): the transposing read of mla_decode_kernel
    const int l15 = lane & 15;
    const int voff = (4 * hh + (l15 >> 2)) * MLA_ROWB + wid * 256 + 32 * (ql >> 4) + 8 * (l15 & 3);
    const int koff = ql * MLA_ROWB + wid * (MLA_WIDTH / 2) + 16 * hh;      // A operand of S^T: row ql, depth 144 wid + 8 hh (+ 16 ks)

    if (tid < MLA_KEYS) {
        rowmap[tid] = resolve(0);
        rowmap[MLA_KEYS + tid] = resolve(1);
    }
    __syncthreads();
    if (nt > 0) {
        load_tile(0);
        store_tile();
    }
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
        const int kv0 = c0 + t * MLA_KEYS;
        if (t + 1 < nt) load_tile(t + 1);
        int next_row = -1;                                   // tile t + 2's row, in flight under the MFMAs
        if (tid < MLA_KEYS) next_row = resolve(t + 2);
        f32x16_fl s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < MLA_KS; ++ks) s = mfma32<T>(*reinterpret_cast<const uint4*>(img + koff + 32 * ks), qf[ks], s);
#pragma unroll
        for (int r = 0; r < 16; ++r) red[(wid * 16 + r) * 64 + lane] = s[r];
        __syncthreads();
        // this lane holds keys kv0 + (r & 3) + 8 (r >> 2) + 4 hh of its column; masked by select, never by arithmetic
        const int ll = limc - kv0 - 4 * hh;
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float v = (red[r * 64 + lane] + red[(16 + r) * 64 + lane]) + (red[(32 + r) * 64 + lane] + red[(48 + r) * 64 + lane]);
            s[r] = (r & 3) + 8 * (r >> 2) <= ll ? v * scale_log2e : -INFINITY;
            mx = fmaxf(mx, s[r]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const float m_use = m_new == -INFINITY ? 0.f : m_new;       // nothing visible so far: p = exp2(-inf) = 0
        const bool moved = __builtin_amdgcn_ballot_w64(m_new != m_run) != 0;
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);   // 1 where the maximum stayed, 0 where it was -inf
        float ls = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] = __builtin_amdgcn_exp2f(s[r] - m_use);
            ls += s[r];
        }
        l_run = l_run * alpha + ls;
        m_run = m_new;
        if (moved) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[i][r] *= alpha;
        }
        // O^T += C^T . P^T: 2 k-steps of 16 keys; element j of the B operand is key 16 ks + 8 (j >> 2) + 4 hh + (j & 3)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const uint4 pb = make_uint4(pack16x2<T>(s[8 * ks + 0], s[8 * ks + 1]), pack16x2<T>(s[8 * ks + 2], s[8 * ks + 3]),
                                        pack16x2<T>(s[8 * ks + 4], s[8 * ks + 5]), pack16x2<T>(s[8 * ks + 6], s[8 * ks + 7]));
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const mla_v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) mla_v4s*)(img + voff + 64 * i + (16 * ks) * MLA_ROWB));
                const mla_v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) mla_v4s*)(img + voff + 64 * i + (16 * ks + 8) * MLA_ROWB));
                const uint2 u0 = __builtin_bit_cast(uint2, lo), u1 = __builtin_bit_cast(uint2, hi);
                o[i] = mfma32<T>(make_uint4(u0.x, u0.y, u1.x, u1.y), pb, o[i]);
            }
        }
        __syncthreads();                 // every wave is done with the image and the partials
        if (t + 1 < nt) store_tile();
        if (tid < MLA_KEYS) rowmap[(t & 1) * MLA_KEYS + tid] = next_row;      // read by load_tile(t + 2), a barrier from here
        __syncthreads();
    }

    // registers 4 g4 .. 4 g4 + 3 of tile i are latent columns 128 wid + 32 i + 8 g4 + 4 hh .. + 3 of this lane's column
    if (!live) return;
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const size_t gcol = (size_t)b * ncols + col;
    if (nchunks == 1) {                  // a column that saw no key (an idle sequence) has l = 0 and stores zeros
        const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
        T* orow = out + gcol * MLA_LATENT + wid * 128 + 4 * hh;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                uint2 x;
                x.x = pack16x2<T>(o[i][4 * g4] * inv, o[i][4 * g4 + 1] * inv);
                x.y = pack16x2<T>(o[i][4 * g4 + 2] * inv, o[i][4 * g4 + 3] * inv);
                *reinterpret_cast<uint2*>(orow + i * 32 + 8 * g4) = x;
            }
    } else {                             // decode_combine's record; an empty chunk's is (-inf, 0, 0), which the merge weighs 0
        float* rec = ws + (gcol * nchunks + blockIdx.y) * MLA_REC;
        if (wid == 0 && hh == 0) {
            rec[0] = m_run * 0.6931471805599453f;
            rec[1] = l_tot;
        }
        float* orec = rec + 2 + wid * 128 + 4 * hh;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                *reinterpret_cast<float2*>(orec + i * 32 + 8 * g4) = make_float2(o[i][4 * g4], o[i][4 * g4 + 1]);
                *reinterpret_cast<float2*>(orec + i * 32 + 8 * g4 + 2) = make_float2(o[i][4 * g4 + 2], o[i][4 * g4 + 3]);
            }
    }
}

// ---- the paged latent writer ---------------------------------------------------------------------------------------------------
// One wave per token.  mla_cache_write_kernel (ops_mla.hip) with the table row read from positions[t] and the destination from
// slot_mapping[t]: every arithmetic expression below is that kernel's, in its order, so a slot holds the bits of row positions[t] of a
// contiguous cache.  A negative slot, a slot beyond the pool and a position outside the table write nothing.
template <class T, class TT>
__global__ __launch_bounds__(256) void mla_paged_write_kernel(const T* kv_a, const T* gamma, const TT* cos_t, const TT* sin_t,
                                                              const int32_t* positions, T* cache, const int32_t* slot_mapping, int n_tokens,
                                                              long long slots, int table_rows, float eps) {
    constexpr int N = Vec<T>::N, features = MLA_LATENT, half = MLA_ROPE / 2;
    static_assert(N * 64 == MLA_LATENT, "one 16-byte vector per lane");
    const int lane = threadIdx.x & 63, s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= n_tokens) return;
    const int slot = slot_mapping[s], row = positions[s];
    if (slot < 0 || slot >= slots || row < 0 || row >= table_rows) return;
    const T* xr = kv_a + (size_t)s * MLA_WIDTH;
    T* orow = cache + (size_t)slot * MLA_WIDTH;
    float v[N];
    float sumsq = 0.f;
    Vec<T> t;
    t.load(xr + lane * N);
    t.to_float(v);
#pragma unroll
    for (int j = 0; j < N; ++j) sumsq += v[j] * v[j];
    const float inv = 1.0f / sqrtf(wave_sum(sumsq) / features + eps);
    Vec<T> g;
    g.load(gamma + lane * N);
    float gf[N], ov[N];
    g.to_float(gf);
#pragma unroll
    for (int j = 0; j < N; ++j) ov[j] = v[j] * inv * gf[j];
    Vec<T> w;
    w.from_float(ov);
    w.store(orow + lane * N);
    if (lane < half) {
        const float c = to_f(cos_t[(size_t)row * MLA_ROPE + lane]);
        const float sn = to_f(sin_t[(size_t)row * MLA_ROPE + lane]);
        const float x0 = to_f(xr[MLA_LATENT + lane]);
        const float x1 = to_f(xr[MLA_LATENT + lane + half]);
        orow[MLA_LATENT + lane] = from_f<T>(x0 * c - x1 * sn);
        orow[MLA_LATENT + lane + half] = from_f<T>(x1 * c + x0 * sn);
    }
}

template <class T>
static pgk_status launch_mla_paged(const void* q, const void* cache, const int32_t* block_tables, const int32_t* context_lens, void* out, void* ws,
                                   int num_seqs, int heads, int q_len, int num_blocks, int block_size, int max_blocks, int max_context,
                                   float scale, hipStream_t st) {
    const int nchunks = mla_paged_chunks(heads, q_len, num_seqs, max_context);
    if (pgk_status r = launch_dyn_lds<mla_paged_kernel<T>>(dim3(mla_col_tiles(heads, q_len), nchunks, num_seqs), 256, MLA_PAGED_LDS, true, st,
                                                           (const T*)q, (const T*)cache, block_tables, context_lens, (T*)out, (float*)ws, heads,
                                                           q_len, block_size, max_blocks, num_blocks, max_context, nchunks,
                                                           scale * 1.4426950408889634f))
        return r;
    if (nchunks > 1) {
        decode_phase2_kernel<T, MLA_LATENT><<<num_seqs * heads * q_len, MLA_LATENT, 0, st>>>((const float*)ws, (T*)out, nchunks);
        PGK_LAUNCH_CHECK();
    }
    return PGK_OK;
}

}  // namespace pgk

using namespace pgk;

extern "C" {

const char* pgk_sdpa_mla_paged_plan(int num_heads, int q_len, int num_seqs, int max_context, pgk_dtype dt, int* grid) {
    if (const char* why = mla_paged_refusal(num_heads, q_len, num_seqs, max_context, dt == PGK_BF16 || dt == PGK_F16)) {
        set_error(PGK_ERR_INVALID, "pgk_sdpa_mla_paged_plan: %s (heads %d, q_len %d, sequences %d, max_context %d, dtype %d)", why, num_heads,
                  q_len, num_seqs, max_context, (int)dt);
        return nullptr;
    }
    if (grid) {
        grid[0] = mla_col_tiles(num_heads, q_len);
        grid[1] = mla_paged_chunks(num_heads, q_len, num_seqs, max_context);
        grid[2] = num_seqs;
    }
    return "mla_paged_mfma";
}

size_t pgk_sdpa_mla_paged_workspace_bytes(int num_heads, int q_len, int num_seqs, int max_context) {
    if (mla_paged_refusal(num_heads, q_len, num_seqs, max_context, true)) return 0;
    const int nchunks = mla_paged_chunks(num_heads, q_len, num_seqs, max_context);
    return nchunks > 1 ? (size_t)num_seqs * num_heads * q_len * nchunks * MLA_REC * sizeof(float) : 0;
}

pgk_status pgk_sdpa_mla_paged(const void* q, const void* cache, const int32_t* block_tables, const int32_t* context_lens, void* out, int num_seqs,
                              int num_heads, int q_len, int num_blocks, int block_size, int max_blocks_per_seq, int max_context, float scale,
                              void* workspace, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(q && cache && block_tables && context_lens && out, "pgk_sdpa_mla_paged: null pointer");
    const char* why = mla_paged_refusal(num_heads, q_len, num_seqs, max_context, dt == PGK_BF16 || dt == PGK_F16);
    PGK_REQUIRE(!why, "pgk_sdpa_mla_paged: %s (heads %d, q_len %d, sequences %d, max_context %d, dtype %d)", why, num_heads, q_len, num_seqs,
                max_context, (int)dt);
    PGK_REQUIRE(num_blocks >= 1 && block_size >= 1 && max_blocks_per_seq >= 1 && (long long)num_blocks * block_size < (1LL << 31),
                "pgk_sdpa_mla_paged: bad pages (num_blocks %d, block_size %d, max_blocks_per_seq %d; under 2^31 rows in all)", num_blocks,
                block_size, max_blocks_per_seq);
    PGK_REQUIRE(scale > 0.f, "pgk_sdpa_mla_paged: scale must be positive (the model's mscale^2 / sqrt(192) has no default), got %g", (double)scale);
    PGK_REQUIRE(aligned16(q) && aligned16(cache) && aligned16(out), "pgk_sdpa_mla_paged: q, cache and out must be 16-byte aligned");
    PGK_REQUIRE(workspace || mla_paged_chunks(num_heads, q_len, num_seqs, max_context) == 1,
                "pgk_sdpa_mla_paged: more than one chunk needs a workspace of pgk_sdpa_mla_paged_workspace_bytes");
    PGK_REQUIRE(!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, "pgk_sdpa_mla_paged: workspace must be 8-byte aligned");
    hipStream_t st = resolve_stream(s);
    if (dt == PGK_BF16)
        return launch_mla_paged<bf16>(q, cache, block_tables, context_lens, out, workspace, num_seqs, num_heads, q_len, num_blocks, block_size,
                                      max_blocks_per_seq, max_context, scale, st);
    return launch_mla_paged<f16>(q, cache, block_tables, context_lens, out, workspace, num_seqs, num_heads, q_len, num_blocks, block_size,
                                 max_blocks_per_seq, max_context, scale, st);
}

pgk_status pgk_mla_paged_cache_write(const void* kv_a, const void* gamma, const void* cos, const void* sin, const int32_t* positions, void* cache,
                                     const int32_t* slot_mapping, int n_tokens, int num_blocks, int block_size, int table_rows, float eps,
                                     int f32_table, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(kv_a && gamma && cos && sin && positions && cache && slot_mapping, "pgk_mla_paged_cache_write: null pointer");
    PGK_REQUIRE(dt == PGK_BF16 || dt == PGK_F16, "pgk_mla_paged_cache_write: bfloat16 / float16 only (dtype %d)", (int)dt);
    PGK_REQUIRE(n_tokens >= 0 && num_blocks >= 1 && block_size >= 1 && table_rows >= 1,
                "pgk_mla_paged_cache_write: bad shape tokens=%d num_blocks=%d block_size=%d table=%d", n_tokens, num_blocks, block_size, table_rows);
    PGK_REQUIRE(aligned16(kv_a) && aligned16(gamma) && aligned16(cache), "pgk_mla_paged_cache_write: kv_a, gamma and cache must be 16-byte aligned");
    if (n_tokens == 0) return PGK_OK;
    hipStream_t st = resolve_stream(s);
    const dim3 grid((unsigned)ceil_div(n_tokens, 4));
    const long long slots = (long long)num_blocks * block_size;
#define PGK_MLA_PAGED_WRITE(T, TT)                                                                                                           \
    mla_paged_write_kernel<T, TT><<<grid, 256, 0, st>>>((const T*)kv_a, (const T*)gamma, (const TT*)cos, (const TT*)sin, positions, (T*)cache, \
                                                        slot_mapping, n_tokens, slots, table_rows, eps)
    if (dt == PGK_BF16) { if (f32_table) PGK_MLA_PAGED_WRITE(bf16, float); else PGK_MLA_PAGED_WRITE(bf16, bf16); }
    else { if (f32_table) PGK_MLA_PAGED_WRITE(f16, float); else PGK_MLA_PAGED_WRITE(f16, f16); }
#undef PGK_MLA_PAGED_WRITE
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

}  // extern "C"
