// FP8 (OCP e4m3) PAGED KV cache: the quantising page writer and the split-KV decode over 8-bit pages.  The packed prefill over the
// same pages is a policy of paged_prefill_kernel (ops_paged_prefill.hip).
//
// Contract: the union of ops_paged.hip's and ops_kv_fp8.hip's.  K / V cache [num_blocks, Hkv, block_size, D] in uint8, one fp32
// scale per kv head for K and one for V, value = e4m3(code) * scale, code = rne_e4m3(clamp(x / scale, +-448)); block_tables
// [num_seqs, max_blocks_per_seq], context_lens [num_seqs] and slot_mapping [tokens] int32 as for the 16-bit pages.
//
// Decode (paged_kv8_attn_kernel).  Workgroup = (KV slice, group of G <= 4 query heads of one kv head, sequence); the slices cut the
// sequence's LIVE context into nsplit runs of whole steps (decode_chunk_len), nsplit = paged_nsplit(max_context).  The walk over a
// run is attn_kv_fp8.hip.h's: D / 16 lanes per row with one 16-byte load of 16 codes each, U position-groups in flight, kv8_consume
// and kv8_block_merge as they are, k_scale in the query premultiply and v_scale on the partial record.  What is new is the issue
// stage: a position's row is table[pos / block_size] * page + (pos % block_size) * D, so every K / V address hangs on a table
// entry.  The lookups run one trip ahead: the table entries of trip t + 1 are requested right after the K / V loads of trip t (vector
// memory returns in issue order, so they arrive behind them, under kv8_consume's conversions and dot products) and are row offsets
// in registers by the time trip t + 1 issues - its 2 U loads leave back to back, no table load in front of any of them.  Every lane
// looks its own positions up (the lanes of a row, and of rows that share a page, hit one address), so any block_size >= 1 and any
// alignment of a wave's rows against the pages is the same code; a power-of-two block_size replaces the division by a shift.
// Positions are clamped to the slice's last live row - nothing at or past ctx is fetched, not a table entry and not a code - and
// the clamped copies are masked by select in kv8_consume.
// Hq / Hkv = 8 runs as two groups of 4 heads: eight heads' states (8 x 18 fp32) and queries (8 x 8 dwords) beside the batch do not
// fit the register file without scratch, and the 16-slot merge would need 66 KiB of LDS.  The second group's K / V bytes come from
// the L2 the first filled (consecutive blockIdx.y).
// One slice (max_context <= 512): the record is merged in LDS and normalised in place - no workspace, no second launch.

#include "attn_kv_fp8.hip.h"
#include "pgk_internal.h"

namespace pgk {

// One lane = 16 elements of one (token, kv head) row of BOTH k_new and v_new [tokens][Hkv][D]: two 16-byte loads and one 16-byte
// store of codes per cache.  slot = physical_block * block_size + offset; a negative slot (padding) or one past the pool is skipped.
template <class T>
__global__ __launch_bounds__(256) void paged_kv8_write_kernel(const T* k_new, const T* v_new, uint8_t* kc, uint8_t* vc, const float* k_scale,
                                                              const float* v_scale, const int32_t* slot_mapping, int n_tokens, int hkv,
                                                              int block_size, int d, long long n_slots) {
    const int lpr = d / 16;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)n_tokens * hkv * lpr) return;
    const int sub = (int)(t % lpr), h = (int)(t / lpr % hkv), tok = (int)(t / lpr / hkv);
    const int slot = slot_mapping[tok];
    if (slot < 0 || slot >= n_slots) return;
    const size_t src = ((size_t)tok * hkv + h) * d + sub * 16;
    const size_t dst = (((size_t)(slot / block_size) * hkv + h) * block_size + slot % block_size) * d + sub * 16;
    *reinterpret_cast<uint4*>(kc + dst) = kv8_quantise16<T>(k_new + src, k_scale[h]);
    *reinterpret_cast<uint4*>(vc + dst) = kv8_quantise16<T>(v_new + src, v_scale[h]);
}

template <class T, int D, int G>
__global__ __launch_bounds__(256) void paged_kv8_attn_kernel(const T* q, const uint8_t* kc, const uint8_t* vc, const float* k_scale,
                                                             const float* v_scale, const int32_t* block_tables, const int32_t* context_lens,
                                                             float* ws, T* out, int num_heads, int num_kv_heads, int block_size, int bs_shift,
                                                             int max_blocks, float scale, int nsplit) {
    constexpr int LPR = D / 16, PPW = 64 / LPR, STEP = kv8_step<D>(), RS = D + 2, U = 4, TRIP = U * STEP;
    __shared__ float lds[17 * G * RS];                          // kv8_block_merge's 16 slots | the record of a single-slice call
    const int split = blockIdx.x, h0 = blockIdx.y * G, seq = blockIdx.z, kvh = h0 / (num_heads / num_kv_heads);
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), sub = lane % LPR, grp = lane / LPR;
    const long long cap = (long long)max_blocks * block_size;
    const int ctx_raw = context_lens[seq];
    const int ctx = ctx_raw < 0 ? 0 : (ctx_raw > cap ? (int)cap : ctx_raw);      // never past the block table
    const int chunk = decode_chunk_len(ctx, nsplit, STEP);
    const int c0 = (int)min((long long)split * chunk, (long long)ctx), c1 = min(c0 + chunk, ctx);

    const float qmul = scale * k_scale[kvh];
    uint32_t qb[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const T* qrow = q + ((size_t)seq * num_heads + h0 + g) * D + sub * 16;
        float f[2][8];
        KVLoad<T>::load8(qrow, f[0]);
        KVLoad<T>::load8(qrow + 8, f[1]);
#pragma unroll
        for (int i = 0; i < 8; ++i) qb[g][i] = pack_bf16x2(f[i >> 2][(2 * i) & 7] * qmul, f[i >> 2][(2 * i + 1) & 7] * qmul);
    }
    KV8State<G> st;
    st.init();

    // ---- issue stage: byte offsets of this lane's U rows of the trip whose loads are next ----------------------------------------
    const int32_t* table = block_tables + (size_t)seq * max_blocks;
    const size_t page_bytes = (size_t)num_kv_heads * block_size * D, head_off = (size_t)kvh * block_size * D + sub * 16;
    const int last = c1 - 1;                                     // the slice's last live row (used only where c0 < c1)
    int pg[U], pin[U];                                           // page and row in the page
    auto lookup = [&](int b0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t p = (uint32_t)min(b0 + wid * PPW + u * STEP + grp, last);
            const uint32_t blk = bs_shift >= 0 ? p >> bs_shift : p / (uint32_t)block_size;
            pin[u] = (int)(p - blk * (uint32_t)block_size);
            pg[u] = table[blk];
        }
    };
    if (c0 < c1) lookup(c0);
    for (int b0 = c0; b0 < c1; b0 += TRIP) {                    // workgroup-uniform trip count
        size_t off[U];
#pragma unroll
        for (int u = 0; u < U; ++u) off[u] = (size_t)pg[u] * page_bytes + head_off + (size_t)pin[u] * D;
        KV8Batch<U> kb;                                          // K rows first, then V rows, as kv8_issue
#pragma unroll
        for (int u = 0; u < U; ++u) kb.k[u] = *reinterpret_cast<const uint4*>(kc + off[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) kb.v[u] = *reinterpret_cast<const uint4*>(vc + off[u]);
        lookup(b0 + TRIP);                                       // past the last trip: the clamp makes it the last live row's entry
        kv8_consume<D, G, U>(kb, b0 + wid * PPW, c1, qb, lane, st);
    }

    float* rec = nsplit == 1 ? lds + 16 * G * RS : ws + (((size_t)seq * num_heads + h0) * nsplit + split) * RS;
    kv8_block_merge<D, G>(st, lds, rec, nsplit == 1 ? (size_t)RS : (size_t)nsplit * RS, v_scale[kvh], lane, wid);
    if (nsplit == 1) {                                           // a sequence with ctx <= 0 has l = 0 and stores zeros
        __syncthreads();
        for (int e = threadIdx.x; e < G * D; e += blockDim.x) {
            const int g = e / D, d = e % D;
            const float l = rec[g * RS + 1];
            out[((size_t)seq * num_heads + h0 + g) * D + d] = from_f<T>(l > 0.f ? rec[g * RS + 2 + d] / l : 0.f);
        }
    }
}

// query heads per workgroup of the decode kernel
static int paged_kv8_group(int hq, int hkv) { return hq / hkv >= 4 ? 4 : hq / hkv; }

}  // namespace pgk

using namespace pgk;

extern "C" {

const char* pgk_paged_kv_fp8_plan(int prefill, int num_seqs, int bound, int num_heads, int num_kv_heads, int head_dim, pgk_dtype dt, int* grid3) {
    const char* op = prefill ? "pgk_paged_attention_prefill_fp8" : "pgk_paged_attention_v1_fp8";
    if (const char* why = paged_prefill_refusal(num_heads, num_kv_heads, head_dim, dt == PGK_BF16 || dt == PGK_F16)) {
        set_error(PGK_ERR_INVALID, "%s: %s (Hq=%d, Hkv=%d, D=%d, dtype %d)", op, why, num_heads, num_kv_heads, head_dim, (int)dt);
        return nullptr;
    }
    if (num_seqs < 1 || num_seqs > PP_MAX_SEQS || bound < 0) {
        set_error(PGK_ERR_INVALID, "%s: bad batch (seqs=%d of at most %d, %s=%d)", op, num_seqs, PP_MAX_SEQS,
                  prefill ? "max_query_len" : "max_context", bound);
        return nullptr;
    }
    if (grid3) {
        const PagedPrefillGrid g = paged_prefill_grid(bound, num_heads, num_kv_heads, num_seqs);
        grid3[0] = prefill ? g.x : paged_nsplit(bound);
        grid3[1] = prefill ? g.y : num_heads / paged_kv8_group(num_heads, num_kv_heads);
        grid3[2] = num_seqs;
    }
    return prefill ? "paged_kv_fp8_prefill_mfma" : "paged_kv_fp8_split";
}

// A single slice (max_context <= 512) is merged and normalised inside the workgroup and needs NO workspace (0 bytes, workspace may
// be NULL); from two slices on, one [m, l, o[D]] fp32 record per (sequence, query head, slice) for decode_phase2_kernel.
size_t pgk_paged_attention_fp8_workspace_bytes(int num_seqs, int num_heads, int head_dim, int max_context) {
    const int nsplit = paged_nsplit(max_context);
    return nsplit == 1 ? 0 : (size_t)num_seqs * num_heads * nsplit * (head_dim + 2) * sizeof(float);
}

pgk_status pgk_paged_cache_write_fp8(const void* k_new, const void* v_new, void* k_cache, void* v_cache, const float* k_scale,
                                     const float* v_scale, const int32_t* slot_mapping, int n_tokens, int num_kv_heads, int num_blocks,
                                     int block_size, int head_dim, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(k_new && v_new && k_cache && v_cache && k_scale && v_scale && slot_mapping, "pgk_paged_cache_write_fp8: null pointer");
    PGK_REQUIRE(n_tokens >= 0 && num_kv_heads >= 1 && num_blocks >= 1 && block_size >= 1,
                "pgk_paged_cache_write_fp8: bad shape (tokens=%d, Hkv=%d, blocks=%d, block=%d)", n_tokens, num_kv_heads, num_blocks, block_size);
    PGK_REQUIRE(head_dim == 64 || head_dim == 128, "pgk_paged_cache_write_fp8: head_dim must be 64 or 128, got %d", head_dim);
    PGK_REQUIRE(dt == PGK_BF16 || dt == PGK_F16, "pgk_paged_cache_write_fp8: K / V must be bfloat16 or float16 (dtype %d)", (int)dt);
    PGK_REQUIRE(aligned16(k_new) && aligned16(v_new) && aligned16(k_cache) && aligned16(v_cache),
                "pgk_paged_cache_write_fp8: K / V and the caches must be 16-byte aligned");
    if (!n_tokens) return PGK_OK;
    hipStream_t st = resolve_stream(s);
    const long long lanes = (long long)n_tokens * num_kv_heads * (head_dim / 16), n_slots = (long long)num_blocks * block_size;
    const dim3 grid((unsigned)ceil_div(lanes, 256));
    if (dt == PGK_BF16)
        paged_kv8_write_kernel<bf16><<<grid, 256, 0, st>>>((const bf16*)k_new, (const bf16*)v_new, (uint8_t*)k_cache, (uint8_t*)v_cache, k_scale,
                                                           v_scale, slot_mapping, n_tokens, num_kv_heads, block_size, head_dim, n_slots);
    else
        paged_kv8_write_kernel<f16><<<grid, 256, 0, st>>>((const f16*)k_new, (const f16*)v_new, (uint8_t*)k_cache, (uint8_t*)v_cache, k_scale,
                                                          v_scale, slot_mapping, n_tokens, num_kv_heads, block_size, head_dim, n_slots);
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

pgk_status pgk_paged_attention_v1_fp8(const void* q, const void* k_cache, const void* v_cache, const float* k_scale, const float* v_scale,
                                      const int32_t* block_tables, const int32_t* context_lens, void* out, int num_seqs, int num_heads,
                                      int num_kv_heads, int head_dim, int block_size, int max_blocks_per_seq, int max_context, float scale,
                                      void* workspace, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(q && k_cache && v_cache && k_scale && v_scale && block_tables && context_lens && out, "pgk_paged_attention_v1_fp8: null pointer");
    PGK_REQUIRE(block_size >= 1 && max_blocks_per_seq >= 1, "pgk_paged_attention_v1_fp8: bad paging (block_size=%d, max_blocks=%d)", block_size,
                max_blocks_per_seq);
    int grid3[3];
    if (!pgk_paged_kv_fp8_plan(0, num_seqs, max_context, num_heads, num_kv_heads, head_dim, dt, grid3)) return PGK_ERR_INVALID;
    PGK_REQUIRE(aligned16(q) && aligned16(k_cache) && aligned16(v_cache), "pgk_paged_attention_v1_fp8: q and the caches must be 16-byte aligned");
    const int nsplit = grid3[0], G = paged_kv8_group(num_heads, num_kv_heads);
    PGK_REQUIRE(nsplit == 1 || workspace, "pgk_paged_attention_v1_fp8: contexts beyond 512 need the workspace of pgk_paged_attention_fp8_workspace_bytes");
    if (scale <= 0.f) scale = 1.0f / sqrtf((float)head_dim);
    int bs_shift = -1;
    if ((block_size & (block_size - 1)) == 0)
        for (bs_shift = 0; (1 << bs_shift) < block_size; ++bs_shift) {}
    hipStream_t st = resolve_stream(s);
    const dim3 grid(grid3[0], grid3[1], grid3[2]);
#define PGK_PA8(TT, DD, GG)                                                                                                              \
    if (head_dim == DD && G == GG) {                                                                                                     \
        paged_kv8_attn_kernel<TT, DD, GG><<<grid, 256, 0, st>>>((const TT*)q, (const uint8_t*)k_cache, (const uint8_t*)v_cache, k_scale, v_scale, \
                                                                block_tables, context_lens, (float*)workspace, (TT*)out, num_heads,       \
                                                                num_kv_heads, block_size, bs_shift, max_blocks_per_seq, scale, nsplit);   \
        if (nsplit > 1) decode_phase2_kernel<TT, DD><<<num_seqs * num_heads, DD, 0, st>>>((const float*)workspace, (TT*)out, nsplit);     \
        PGK_LAUNCH_CHECK();                                                                                                              \
        return PGK_OK;                                                                                                                   \
    }
#define PGK_PA8_T(TT) PGK_PA8(TT, 128, 1) PGK_PA8(TT, 128, 2) PGK_PA8(TT, 128, 4) PGK_PA8(TT, 64, 1) PGK_PA8(TT, 64, 2) PGK_PA8(TT, 64, 4)
    if (dt == PGK_BF16) { PGK_PA8_T(bf16) } else { PGK_PA8_T(f16) }
#undef PGK_PA8_T
#undef PGK_PA8
    return set_error(PGK_ERR_INVALID, "pgk_paged_attention_v1_fp8: no kernel for D=%d G=%d", head_dim, G);
}

}  // extern "C"
