// Multi-head latent attention (DeepSeek-V2 / V3 / R1, Kimi-K2) in its absorbed decode form over a latent cache [max_seq][576]:
// row r = [c_r (512, the RMS-normed compressed latent) | kpe_r (64, the roped shared key)], one row for ALL heads.
//   pgk_mla_cache_write        kv_a [S][576] -> rows pos .. pos + S - 1: rmsnorm of the first 512 columns, RoPE of the last 64
//   pgk_sdpa_mla_fixed_cache   out[i][h] = sum_r softmax_r(scale <q[i][h], cache[r]>) cache[r][:512], r <= ctx - q_len + i
//
// The attention kernel (mla_decode_kernel).  A column of the score tile is a (query row, head) pair, column c = row c / H, head
// c % H, so a decode step of 128 heads is four 32-column tiles and a tile may straddle query rows: the causal limit is per column
// (per lane).  Grid (column tiles, cache chunks), 4 waves.  A KV tile is 32 latent rows staged ONCE into LDS, row-major
// [32][576] 16-bit with 16 bytes of padding per row (MLA_ROWB: rows r, r + 1 then start 36 dwords apart modulo the 64 banks and the
// 16-byte operand reads of 8 neighbouring rows fall on 8 different bank quads) - 1152 bytes per key from HBM serve every head - and
// the same image feeds both products, in the orientation of the flash kernels (a lane owns one column for the whole walk):
//   S^T = C . Q^T   contraction 576, SPLIT OVER THE CONTRACTION: wave w takes depth 144 w .. 144 w + 143 (9 k-steps of
//                   v_mfma_f32_32x32x16), its 32 x 144 slice of Q^T lives in 36 VGPRs for the whole walk (the whole fragment
//                   would be 144), the four partial 32 x 32 score tiles meet in LDS (16 KiB) and every wave sums them in the same
//                   order, so all four hold bit-identical scores and run the same fp32 exp2-domain online softmax redundantly;
//   O^T += C[:, :512]^T . P^T   SPLIT OVER THE OUTPUT: wave w owns latent columns 128 w .. 128 w + 127 (4 accumulator tiles, 64
//                   fp32 registers); the A operand C^T comes out of the row-major image through ds_read_b64_tr_b16, the B operand
//                   is the probabilities packed to 16 bits straight from the score registers (key order permuted on both sides).
// Q in LDS instead (the other candidate) would free 36 VGPRs and cost 9 more 16-byte LDS reads per wave and tile on the pipe
// that already carries both operands of both products; the registers are there (228 VGPRs, no scratch, under the bound of two
// workgroups per CU; one image + the partials = 52.5 KiB of LDS would allow three), so Q stays in registers.
// Staging: a tile is 2304 16-byte chunks, 9 per thread; the chunks of tile t + 1 are in flight (registers) under the MFMAs of
// tile t and stored after them - one image, three barriers per tile.  Rows at or beyond the end of the chunk's live range
// (never past the context) are not loaded: their image rows are zero, their scores masked by select, so no byte of a row at or
// beyond the context ever enters a product - 0 x NaN inside an MFMA is NaN, which is why the VALUE side is zeroed too.  Rows
// below the context but above a column's own limit are live rows of later query rows: their probabilities are exactly 0.
// Split-KV: chunk k of mla_chunks(..) covers rows [k L, (k + 1) L) of the context, L = decode_chunk_len(ctx, chunks, 32).  With one
// chunk the kernel normalises and writes `out`; otherwise it leaves the record (m ln 2, l, O[512]) of decode_phase1_kernel per
// (column, chunk) and decode_phase2_kernel<T, 512> (attn_core.hip.h), one block per column, merges them.

#include "attn_core.hip.h"
#include "flash_common.hip.h"
#include "pgk_internal.h"

namespace pgk {

constexpr int MLA_ROWB = MLA_WIDTH * 2 + 16;                 // bytes per image row
constexpr int MLA_IMG = MLA_KEYS * MLA_ROWB;                 // 37376
constexpr int MLA_RED = 4 * 16 * 64 * 4;                     // partial scores: [wave][register][lane] fp32
constexpr int MLA_LDS = MLA_IMG + MLA_RED;
constexpr int MLA_STAGE = MLA_KEYS * (MLA_WIDTH / 8) / 256;  // 16-byte chunks a thread stages per tile
constexpr int MLA_KS = MLA_WIDTH / 4 / 16;                   // k-steps of a wave's quarter of the contraction
constexpr int MLA_REC = MLA_LATENT + 2;
static_assert(MLA_STAGE * 256 == MLA_KEYS * (MLA_WIDTH / 8) && MLA_KS * 64 == MLA_WIDTH && MLA_COLS == 32 && MLA_KEYS == 32, "mla tile");

typedef short mla_v4s __attribute__((ext_vector_type(4)));

template <class T>
__global__ __launch_bounds__(256, 2) void mla_decode_kernel(const T* q, const T* cache, T* out, float* ws, int heads, int q_len, int max_seq,
                                                         int nchunks, float scale_log2e, int host_ctx, const int32_t* ctx_buf) {
    extern __shared__ __attribute__((aligned(16))) char mla_smem[];      // image | partial scores
    char* img = mla_smem;
    float* red = reinterpret_cast<float*>(mla_smem + MLA_IMG);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, ql = lane & 31, hh = lane >> 5;
    const int ctx = max(min(ctx_buf ? ctx_buf[0] : host_ctx, max_seq), 0);
    const int ncols = heads * q_len, col0 = blockIdx.x * MLA_COLS, col = col0 + ql;
    const bool live = col < ncols;                           // a tail column: zero query, never stored
    const int moff = ctx - q_len;                            // query row i sees keys <= moff + i
    const int lim = moff + min(col, ncols - 1) / heads;
    const int kv_end = max(moff + min(col0 + MLA_COLS - 1, ncols - 1) / heads + 1, 0);      // keys the tile's last live column sees (<= ctx)
    const int clen = decode_chunk_len(ctx, nchunks, MLA_KEYS);
    const int c0 = min((int)blockIdx.y * clen, kv_end), c1 = min(c0 + clen, kv_end);
    const int nt = (c1 - c0 + MLA_KEYS - 1) / MLA_KEYS;
    const int limc = min(lim, c1 - 1);

    // Q^T fragments (B operand): lane = column, k = depth 144 wid + 16 ks + 8 hh .. + 7, the caller's bits: scale * log2(e) multiplies
    // the fp32 scores, so the query is never rounded a second time
    uint4 qf[MLA_KS];
    {
        const T* qrow = q + (size_t)min(col, ncols - 1) * MLA_WIDTH + wid * (MLA_WIDTH / 4) + 8 * hh;
#pragma unroll
        for (int ks = 0; ks < MLA_KS; ++ks) qf[ks] = live ? *reinterpret_cast<const uint4*>(qrow + ks * 16) : make_uint4(0, 0, 0, 0);
    }
    f32x16_fl o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    // ---- staging: chunk tid + 256 j of the tile's 2304, row (tid + 256 j) / 72; zero at or beyond c1 ------------------------------
    uint4 st[MLA_STAGE];
    auto load_tile = [&](int t) {
        const int row0 = c0 + t * MLA_KEYS;
#pragma unroll
        for (int j = 0; j < MLA_STAGE; ++j) {
            const int c = tid + 256 * j, r = c / (MLA_WIDTH / 8), cc = c % (MLA_WIDTH / 8);
            st[j] = make_uint4(0, 0, 0, 0);
            if (row0 + r < c1) st[j] = *reinterpret_cast<const uint4*>(cache + (size_t)(row0 + r) * MLA_WIDTH + cc * 8);
        }
    };
    auto store_tile = [&] {
#pragma unroll
        for (int j = 0; j < MLA_STAGE; ++j) {
            const int c = tid + 256 * j, r = c / (MLA_WIDTH / 8), cc = c % (MLA_WIDTH / 8);
            *reinterpret_cast<uint4*>(img + r * MLA_ROWB + cc * 16) = st[j];
        }
    };
    // C^T fragment of (k-step s, half u, latent tile i of this wave): paged_prefill_kernel's transposing read - the 16 lanes of a
    // quarter-wave read the 4 x 16 block of rows 16 s + 8 u + 4 hh + (0..3), columns 128 wid + 32 i + 16 (ql >> 4) + (0..15)
    const int l15 = lane & 15;
    const int voff = (4 * hh + (l15 >> 2)) * MLA_ROWB + wid * 256 + 32 * (ql >> 4) + 8 * (l15 & 3);
    const int koff = ql * MLA_ROWB + wid * (MLA_WIDTH / 2) + 16 * hh;      // A operand of S^T: row ql, depth 144 wid + 8 hh (+ 16 ks)

    if (nt > 0) {
        load_tile(0);
        store_tile();
    }
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
        const int kv0 = c0 + t * MLA_KEYS;
        if (t + 1 < nt) load_tile(t + 1);
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
        __syncthreads();
    }

    // registers 4 g4 .. 4 g4 + 3 of tile i are latent columns 128 wid + 32 i + 8 g4 + 4 hh .. + 3 of this lane's column
    if (!live) return;
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    if (nchunks == 1) {                  // a column that saw no key has l = 0 and untouched accumulators and stores zeros
        const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
        T* orow = out + (size_t)col * MLA_LATENT + wid * 128 + 4 * hh;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                uint2 x;
                x.x = pack16x2<T>(o[i][4 * g4] * inv, o[i][4 * g4 + 1] * inv);
                x.y = pack16x2<T>(o[i][4 * g4 + 2] * inv, o[i][4 * g4 + 3] * inv);
                *reinterpret_cast<uint2*>(orow + i * 32 + 8 * g4) = x;
            }
    } else {                             // decode_combine's record: m in the natural-log domain, l, the unnormalised O
        float* rec = ws + ((size_t)col * nchunks + blockIdx.y) * MLA_REC;
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

// ---- the latent cache writer ---------------------------------------------------------------------------------------------------
// One wave per row of kv_a.  Columns 0 .. 511: norm_wave_kernel's rmsnorm at 512 features (ops_norm_rope.hip) - one 16-byte vector
// per lane, the same sum of squares in the same order through wave_sum, the same v * inv * gamma.  Columns 512 .. 575: rope_kernel's
// rotate-half of the pair (d, d + 32) at table row pos + s, lanes 0 .. 31.  The bits are those of rmsnorm + rope_inplace + a copy.
// A row outside the cache or the table is not written (a device-resident position is not checked by the host).
template <class T, class TT>
__global__ __launch_bounds__(256) void mla_cache_write_kernel(const T* kv_a, const T* gamma, const TT* cos_t, const TT* sin_t, T* cache, int seq,
                                                              int max_seq, int table_rows, float eps, int host_pos, const int32_t* pos_buf) {
    constexpr int N = Vec<T>::N, features = MLA_LATENT, half = MLA_ROPE / 2;
    static_assert(N * 64 == MLA_LATENT, "one 16-byte vector per lane");
    const int lane = threadIdx.x & 63, s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= seq) return;
    const long long row = (long long)(pos_buf ? pos_buf[0] : host_pos) + s;
    if (row < 0 || row >= max_seq || row >= table_rows) return;
    const T* xr = kv_a + (size_t)s * MLA_WIDTH;
    T* orow = cache + (size_t)row * MLA_WIDTH;
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
static pgk_status launch_mla_decode(const void* q, const void* cache, void* out, void* ws, int heads, int q_len, int max_seq, float scale,
                                    int h_ctx, const int32_t* ctx_buf, hipStream_t st) {
    const int nchunks = mla_chunks(heads, q_len, max_seq);
    if (pgk_status r = launch_dyn_lds<mla_decode_kernel<T>>(dim3(mla_col_tiles(heads, q_len), nchunks), 256, MLA_LDS, true, st, (const T*)q,
                                                            (const T*)cache, (T*)out, (float*)ws, heads, q_len, max_seq, nchunks,
                                                            scale * 1.4426950408889634f, h_ctx, ctx_buf))
        return r;
    if (nchunks > 1) {
        decode_phase2_kernel<T, MLA_LATENT><<<heads * q_len, MLA_LATENT, 0, st>>>((const float*)ws, (T*)out, nchunks);
        PGK_LAUNCH_CHECK();
    }
    return PGK_OK;
}

}  // namespace pgk

using namespace pgk;

extern "C" {

const char* pgk_sdpa_mla_plan(int num_heads, int q_len, int max_seq, pgk_dtype dt, int* cols, int* chunks) {
    if (const char* why = mla_refusal(num_heads, q_len, max_seq, dt == PGK_BF16 || dt == PGK_F16)) {
        set_error(PGK_ERR_INVALID, "pgk_sdpa_mla_plan: %s (heads %d, q_len %d, rows %d, dtype %d)", why, num_heads, q_len, max_seq, (int)dt);
        return nullptr;
    }
    if (cols) *cols = MLA_COLS;
    if (chunks) *chunks = mla_chunks(num_heads, q_len, max_seq);
    return "mla_latent_mfma";
}

size_t pgk_sdpa_mla_workspace_bytes(int num_heads, int q_len, int max_seq) {
    if (mla_refusal(num_heads, q_len, max_seq, true)) return 0;
    const int nchunks = mla_chunks(num_heads, q_len, max_seq);
    return nchunks > 1 ? (size_t)num_heads * q_len * nchunks * MLA_REC * sizeof(float) : 0;
}

pgk_status pgk_sdpa_mla_fixed_cache(const void* q, const void* cache, void* out, int num_heads, int q_len, int max_seq, float scale,
                                    int h_context_len, const int32_t* ctx_buf, void* workspace, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(q && cache && out, "pgk_sdpa_mla_fixed_cache: null pointer");
    const char* why = mla_refusal(num_heads, q_len, max_seq, dt == PGK_BF16 || dt == PGK_F16);
    PGK_REQUIRE(!why, "pgk_sdpa_mla_fixed_cache: %s (heads %d, q_len %d, rows %d, dtype %d)", why, num_heads, q_len, max_seq, (int)dt);
    PGK_REQUIRE(scale > 0.f, "pgk_sdpa_mla_fixed_cache: scale must be positive (the model's mscale^2 / sqrt(192) has no default), got %g",
                (double)scale);
    PGK_REQUIRE(ctx_buf || (h_context_len >= q_len && h_context_len <= max_seq),
                "pgk_sdpa_mla_fixed_cache: invalid context_len %d (q_len %d, cache rows %d)", h_context_len, q_len, max_seq);
    PGK_REQUIRE(aligned16(q) && aligned16(cache) && aligned16(out), "pgk_sdpa_mla_fixed_cache: q, cache and out must be 16-byte aligned");
    PGK_REQUIRE(workspace || mla_chunks(num_heads, q_len, max_seq) == 1,
                "pgk_sdpa_mla_fixed_cache: more than one chunk needs a workspace of pgk_sdpa_mla_workspace_bytes");
    PGK_REQUIRE(!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, "pgk_sdpa_mla_fixed_cache: workspace must be 8-byte aligned");
    hipStream_t st = resolve_stream(s);
    if (dt == PGK_BF16) return launch_mla_decode<bf16>(q, cache, out, workspace, num_heads, q_len, max_seq, scale, h_context_len, ctx_buf, st);
    return launch_mla_decode<f16>(q, cache, out, workspace, num_heads, q_len, max_seq, scale, h_context_len, ctx_buf, st);
}

pgk_status pgk_mla_cache_write(const void* kv_a, const void* gamma, const void* cos, const void* sin, void* cache, int seq, int max_seq,
                               int table_rows, float eps, int h_pos, const int32_t* pos_buf, int f32_table, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(kv_a && gamma && cos && sin && cache, "pgk_mla_cache_write: null pointer");
    PGK_REQUIRE(dt == PGK_BF16 || dt == PGK_F16, "pgk_mla_cache_write: bfloat16 / float16 only (dtype %d)", (int)dt);
    PGK_REQUIRE(seq >= 0 && max_seq >= 1 && table_rows >= 1, "pgk_mla_cache_write: bad shape seq=%d rows=%d table=%d", seq, max_seq, table_rows);
    PGK_REQUIRE(pos_buf || (h_pos >= 0 && (long long)h_pos + seq <= max_seq && (long long)h_pos + seq <= table_rows),
                "pgk_mla_cache_write: rows %d..%lld outside the cache of %d rows or the table of %d", h_pos, (long long)h_pos + seq - 1, max_seq,
                table_rows);
    PGK_REQUIRE(aligned16(kv_a) && aligned16(gamma) && aligned16(cache), "pgk_mla_cache_write: kv_a, gamma and cache must be 16-byte aligned");
    if (seq == 0) return PGK_OK;
    hipStream_t st = resolve_stream(s);
    const dim3 grid((unsigned)ceil_div(seq, 4));
#define PGK_MLA_WRITE(T, TT)                                                                                                              \
    mla_cache_write_kernel<T, TT><<<grid, 256, 0, st>>>((const T*)kv_a, (const T*)gamma, (const TT*)cos, (const TT*)sin, (T*)cache, seq, max_seq, \
                                                        table_rows, eps, h_pos, pos_buf)
    if (dt == PGK_BF16) { if (f32_table) PGK_MLA_WRITE(bf16, float); else PGK_MLA_WRITE(bf16, bf16); }
    else { if (f32_table) PGK_MLA_WRITE(f16, float); else PGK_MLA_WRITE(f16, f16); }
#undef PGK_MLA_WRITE
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

}  // extern "C"
