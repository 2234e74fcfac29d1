// Packed variable-length prefill attention over the paged KV cache (bf16 / f16 queries over 16-bit or FP8 e4m3 pages, head_dim 64 or
// 128, Hq / Hkv in {1, 2, 4, 8}).
//
// out[row] = softmax(scale . q[row] K^T + causal mask) V for a packed batch q [total_tokens, Hq, D]: the rows of sequence b are
// cu_seqlens_q[b] .. cu_seqlens_q[b + 1] - 1, its keys are the first context_lens[b] logical positions of its pages
// (block_tables[b][pos / block_size], row pos % block_size of K / V cache [num_blocks, Hkv, block_size, D]), and local row i
// sees key j iff j <= context_lens[b] - q_len_b + i.  Whole prompts, chunks behind a cached prefix, decode rows (q_len 1) and
// idle sequences (q_len 0) share one launch; every length stays on the device, the grid is sized by max_query_len alone.
//
// Work split.  A column of the score tile is a (query position, query head of the kv head's group) pair: column c of a sequence
// is position c / G, head c % G.  A workgroup of 4 waves owns 128 consecutive columns - 128 / G positions x the G heads of ONE kv
// head - so every 64-key tile of K and V is staged into LDS once per kv head and serves all G query heads, and a decode row fills
// G columns instead of one.  Grid (ceil(max_query_len G / 128), Hkv, num_seqs), its ids re-dealt inside the kernel (below); a
// workgroup past its sequence's last column returns before the first barrier.
// Orientation is the second-generation flash kernel's (flash_core.hip.h): S^T = K . Q^T on v_mfma_f32_32x32x16, a lane owns one
// column for the whole walk, online softmax in fp32 in the exp2 domain with the deferred rescale, O^T += V^T . P^T on the same
// MFMA with the packed probabilities as the B operand straight from the score registers.
// K / V staging.  The 64 rows of a tile are looked up one by one - page = block_tables[b][pos / block_size], so any block_size
// >= 1 and any alignment of tile against page works - clamped to position ctx - 1: a row at or past ctx is a copy of a live row
// and its scores are masked by select, so stale cache contents (NaN / Inf in freed pages and in the tail of the last page) never
// enter a product.  K goes into the XOR-swizzled [64][D] image of the flash kernel (fl_k_off, ops_flash.hip).  V is staged
// ROW-MAJOR, [64][D] as well, and becomes the A operand V^T through gfx950's transposing LDS read (ds_read_b64_tr_b16): there is
// no V^T workspace, no pre-pass and no allocation.  The page numbers of tile t + 2 and the K / V rows of tile t + 1 are in
// flight (registers) under the MFMAs of tile t; both images are double buffered in LDS (64 KiB at D = 128, 32 KiB at D = 64).
// The pages hold the kernel's 16-bit type or e4m3 codes (PagedKV16 / PagedKV8 below): one kernel, two stagings.
// No KV split: a decode row over a very long context is one workgroup's walk (pgk_paged_attention_v1 is the pure-decode tool).

#include "flash_common.hip.h"
#include "pgk_internal.h"

namespace pgk {

// K image: fl_k_off of ops_flash.hip - [64 kv][D] 16-bit, 16-byte chunk c of row r at r * 2D + ((c ^ (r & (D/8 - 1))) << 4)
template <int D> __device__ __forceinline__ int pp_k_off(int r, int c) { return r * (2 * D) + ((c ^ (r & (D / 8 - 1))) << 4); }

// V image: [64 kv][D] 16-bit row-major, rows of 2D bytes cut into 64-byte segments (32 dims); segment g of row r sits at segment
// g ^ sw(r), sw(r) = r & 3 at D = 128 and (r >> 1) & 1 at D = 64.  A transposing read of one half-wave covers 4 consecutive rows
// (r0 a multiple of 4) x one segment: at D = 128 the four rows' segments are four different ones of a 256-byte row, at D = 64
// rows r0, r0 + 1 are the two 128-byte halves of a 256-byte line and rows r0 + 2, r0 + 3 take the other segment of each - the
// 256 bytes of a half-wave fall on 64 different banks either way.  A 16-byte staging store keeps its chunk inside its segment.
template <int D> __device__ __forceinline__ int pp_v_sw(int r) { return D == 128 ? (r & 3) : ((r >> 1) & 1); }
template <int D> __device__ __forceinline__ int pp_v_off(int r, int c) { return r * (2 * D) + (((c >> 2) ^ pp_v_sw<D>(r)) << 6) + ((c & 3) << 4); }

typedef short pp_v4s __attribute__((ext_vector_type(4)));

// What the pages hold: last template argument and last argument of paged_prefill_kernel, as FlashPlain / FlashIrope are
// flash_fwd_kernel's.  PagedKV16: words of the kernel's own 16-bit type.  PagedKV8 (pgk_paged_attention_prefill_fp8): OCP e4m3
// codes with one fp32 scale per kv head for K and one for V.  Only the staging differs.  A K / V row is D BYTES in global memory,
// so a 16-byte load brings 16 codes and a tile needs half as many load instructions (and page lookups): a thread stages D / 64
// rows per image and tile instead of D / 32, D / 16 threads to a row.  The codes wait in registers under the MFMAs of the tile
// before (one uint4 per row, half of what the 16-bit words take) and are converted where they are stored: v_cvt_scalef32_pk_bf16_fp8
// / _pk_f16_fp8 with scale 1 - exact, e4m3 is a subset of both types - give the two 16-byte chunks 2 sc, 2 sc + 1 of the SAME
// swizzled K image and row-major V image, so the MFMA operand reads and ds_read_b64_tr_b16 do not know the difference.  k_scale
// joins scale . log2(e) in the Q premultiply and v_scale the final 1 / l; the walk never sees either.
// Which of its two chunks a thread stores first depends on its row (pp_first): the 16 lanes that share a pass of a 16-byte LDS
// store then cover 256 different bytes modulo the 64 banks, as the 16-bit staging's 16 consecutive chunks do.  In the K image
// at D = 128 the row's own XOR already does that (rows r, r + 1 flip the parity of chunk 2 sc); in the V image, whose swizzle moves
// whole 64-byte segments, and in both images at D = 64, where rows r and r + 2 share a 128-byte half line, it is the row bit that
// separates the two rows.
struct PagedKV16 { static constexpr bool fp8 = false; };
struct PagedKV8 { static constexpr bool fp8 = true; const float* k_scale; const float* v_scale; };

template <class T> __device__ __forceinline__ uint32_t pp_cvt2(uint32_t w, bool hi);
template <> __device__ __forceinline__ uint32_t pp_cvt2<bf16>(uint32_t w, bool hi) {
    return hi ? __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true))
              : __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false));
}
template <> __device__ __forceinline__ uint32_t pp_cvt2<f16>(uint32_t w, bool hi) {
    return hi ? __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, true))
              : __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, false));
}
// 8 codes (two dwords) -> one 16-byte chunk of T, element order kept
template <class T> __device__ __forceinline__ uint4 pp_cvt8(uint32_t a, uint32_t b) {
    return make_uint4(pp_cvt2<T>(a, false), pp_cvt2<T>(a, true), pp_cvt2<T>(b, false), pp_cvt2<T>(b, true));
}
__device__ __forceinline__ uint4 pp_pick(bool second, const uint4& a, const uint4& b) {
    return make_uint4(second ? b.x : a.x, second ? b.y : a.y, second ? b.z : a.z, second ? b.w : a.w);
}
// which chunk of its pair (0: 2 sc, 1: 2 sc + 1) the thread staging row r stores first, K image / V image
template <int D> __device__ __forceinline__ int pp_first_k(int r) { return D == 128 ? 0 : (r >> 1) & 1; }
template <int D> __device__ __forceinline__ int pp_first_v(int r) { return D == 128 ? r & 1 : (r >> 1) & 1; }

template <class T, int D, int G, class KV = PagedKV16>
__global__ __launch_bounds__(256, 2) void paged_prefill_kernel(const T* q, const typename std::conditional<KV::fp8, uint8_t, T>::type* kc,
                                                               const typename std::conditional<KV::fp8, uint8_t, T>::type* vc,
                                                               const int32_t* block_tables,
                                                               const int32_t* context_lens, const int32_t* cu_seqlens_q, T* out,
                                                               int total_tokens, int num_heads, int num_kv_heads, int block_size,
                                                               int bs_shift, int max_blocks, float scale_log2e, KV kv) {
    constexpr int EPC = KV::fp8 ? 16 : 8; // cache elements per 16-byte chunk of global memory
    constexpr int NC = D / EPC;          // 16-byte chunks per K / V row in global memory
    constexpr int KS = D / 16;           // k-steps of K . Q^T
    constexpr int DT = D / 32;           // 32-row tiles of O^T
    constexpr int CH = NC / 4;           // rows (one chunk of each) a thread stages per image and tile
    constexpr int R_STEP = 256 / NC;     // row distance between a thread's chunks
    constexpr int IMG = 64 * D * 2;      // bytes of one K or V image
    static_assert(D == 64 || D == 128, "head_dim 64 / 128");
    extern __shared__ __attribute__((aligned(16))) char pp_smem[];   // K[2] | V[2]

    // Workgroup id -> (kv head, sequence, column tile), kv head fastest, then the sequence, the column tiles from the last down.
    // The dispatcher deals consecutive ids to the 8 XCDs in turn, so (a) with Hkv a multiple of 8 a kv head's K / V stream is
    // served by one L2, (b) the live workgroups of the short sequences of a mixed batch - tile 0 of each decode row - are
    // consecutive ids and spread over every XCD (as blockIdx.x = 0 of a grid row of 32 ids they all landed on ONE: measured 1230 us
    // against 139 us for 3 x 1024-token prompts + 32 decode rows at context 2048), and (c) the late column tiles of long prompts,
    // which see the most keys, start first.
    const int wg = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z), rest = wg / num_kv_heads;
    const int kvh = wg % num_kv_heads, seq = rest % (int)gridDim.z, col0 = ((int)gridDim.x - 1 - rest / (int)gridDim.z) * PP_COLS;
    const int q0 = cu_seqlens_q[seq], q_len = cu_seqlens_q[seq + 1] - q0;
    if (col0 >= q_len * G) return;       // idle sequence, or past its last column tile (workgroup-uniform, before any barrier)
    const long long cap = (long long)max_blocks * block_size;
    const int ctx_raw = context_lens[seq];
    const int ctx = ctx_raw < 0 ? 0 : (ctx_raw > cap ? (int)cap : ctx_raw);      // never past the block table
    const int moff = ctx - q_len;        // local row i sees key j <= moff + i

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, ql = lane & 31, h = lane >> 5;
    const int wcol0 = col0 + wid * 32, col = wcol0 + ql;
    const int pos_raw = col / G, hg = col % G;
    const int pos = min(pos_raw, q_len - 1);                 // a column past the sequence computes a copy of its last row, unstored
    const int lim = moff + pos;                              // last visible key of this column (<= ctx - 1; < 0: none)
    const int lim_first = moff + min(wcol0 / G, q_len - 1);  // of the wave's first and last column (wave-uniform)
    const int lim_last = moff + min((wcol0 + 31) / G, q_len - 1);
    const int kv_end = moff + min((col0 + PP_COLS - 1) / G, q_len - 1) + 1;      // keys the workgroup's last live column sees (<= ctx)
    const int nt = kv_end > 0 ? (kv_end + 63) >> 6 : 0;
    const long long tok = (long long)q0 + pos;
    const bool store_ok = pos_raw < q_len && tok >= 0 && tok < total_tokens;
    const size_t row_off = ((size_t)min(max(tok, 0LL), (long long)total_tokens - 1) * num_heads + kvh * G + hg) * D;

    // Q^T fragments (B operand): lane = column, k = d; premultiplied by scale * log2(e) (one more rounding to 16 bits, as the flash
    // kernel), so the scores leave the MFMA in the exp2 domain
    uint4 qf[KS];
    float qmul = scale_log2e;
    if constexpr (KV::fp8) qmul *= kv.k_scale[kvh];
    {
        const T* qrow = q + row_off + 8 * h;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            Vec<T> v;
            v.load(qrow + ks * 16);
            float f[8];
            v.to_float(f);
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] *= qmul;
            v.from_float(f);
            qf[ks] = v.raw;
        }
    }
    f32x16_fl o[DT];
#pragma unroll
    for (int i = 0; i < DT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    // ---- staging: chunk sc of rows sr + R_STEP i of a tile; their page and row-in-page one tile ahead of their K / V loads --------
    const int sr = tid / NC, sc = tid % NC;
    const int32_t* table = block_tables + (size_t)seq * max_blocks;
    const size_t page_elems = (size_t)num_kv_heads * block_size * D, head_off = (size_t)kvh * block_size * D + sc * EPC;
    // named registers, not arrays: at this register pressure hipcc leaves an array of staged chunks in scratch memory (FlashVStage)
    static_assert(CH == 1 || CH == 2 || CH == 4, "staging is written for D = 64 / 128");
    int pg0 = 0, pg1 = 0, pg2 = 0, pg3 = 0, pin0 = 0, pin1 = 0, pin2 = 0, pin3 = 0;      // of the tile whose K / V loads are next
    uint4 rk0, rk1, rk2, rk3, rv0, rv1, rv2, rv3;
    auto page_of = [&](int t, int i, int& page, int& in_page) {
        const uint32_t p = (uint32_t)min(t * 64 + sr + R_STEP * i, ctx - 1);      // ctx >= 1 whenever a tile exists
        const uint32_t blk = bs_shift >= 0 ? p >> bs_shift : p / (uint32_t)block_size;
        in_page = (int)(p - blk * (uint32_t)block_size);
        page = table[blk];
    };
    auto load_pages = [&](int t) {
        page_of(t, 0, pg0, pin0);
        if constexpr (CH >= 2) page_of(t, 1, pg1, pin1);
        if constexpr (CH == 4) { page_of(t, 2, pg2, pin2); page_of(t, 3, pg3, pin3); }
    };
    auto row_of = [&](int page, int in_page, uint4& k, uint4& v) {
        const size_t off = (size_t)page * page_elems + head_off + (size_t)in_page * D;
        k = *reinterpret_cast<const uint4*>(kc + off);
        v = *reinterpret_cast<const uint4*>(vc + off);
    };
    auto load_kv = [&] {
        row_of(pg0, pin0, rk0, rv0);
        if constexpr (CH >= 2) row_of(pg1, pin1, rk1, rv1);
        if constexpr (CH == 4) { row_of(pg2, pin2, rk2, rv2); row_of(pg3, pin3, rk3, rv3); }
    };
    auto store_kv = [&](int buf) {
        char* kb = pp_smem + buf * IMG;
        char* vb = pp_smem + (2 + buf) * IMG;
        auto put = [&](int i, const uint4& k, const uint4& v) {
            if constexpr (KV::fp8) {     // R_STEP is a multiple of 4: the row bits of pp_first are the thread's own
                const int r = sr + R_STEP * i, fk = pp_first_k<D>(sr), fv = pp_first_v<D>(sr);
                const uint4 k0 = pp_cvt8<T>(k.x, k.y), k1 = pp_cvt8<T>(k.z, k.w), v0 = pp_cvt8<T>(v.x, v.y), v1 = pp_cvt8<T>(v.z, v.w);
                *reinterpret_cast<uint4*>(kb + pp_k_off<D>(r, 2 * sc + fk)) = pp_pick(fk, k0, k1);
                *reinterpret_cast<uint4*>(kb + pp_k_off<D>(r, 2 * sc + 1 - fk)) = pp_pick(!fk, k0, k1);
                *reinterpret_cast<uint4*>(vb + pp_v_off<D>(r, 2 * sc + fv)) = pp_pick(fv, v0, v1);
                *reinterpret_cast<uint4*>(vb + pp_v_off<D>(r, 2 * sc + 1 - fv)) = pp_pick(!fv, v0, v1);
            } else {
                *reinterpret_cast<uint4*>(kb + pp_k_off<D>(sr + R_STEP * i, sc)) = k;
                *reinterpret_cast<uint4*>(vb + pp_v_off<D>(sr + R_STEP * i, sc)) = v;
            }
        };
        put(0, rk0, rv0);
        if constexpr (CH >= 2) put(1, rk1, rv1);
        if constexpr (CH == 4) { put(2, rk2, rv2); put(3, rk3, rv3); }
    };
    // V^T fragment of (k-step s, half u, dim tile i): the 16 lanes of a quarter-wave read the 4 x 16 block of rows
    // 16 s + 8 u + 4 h + (0..3), dims 32 i + 16 (ql >> 4) + (0..15); lane l15 addresses row l15 >> 2, dims 4 (l15 & 3) .. + 4 of it
    // and receives the four rows of dim l15 - k-slots (j & 3) of the order the probabilities are packed in.  The row's swizzle
    // term depends on l15 alone, so the address is a per-lane base per dim tile plus a literal.
    int voff[DT];
    {
        const int l15 = lane & 15, r = 4 * h + (l15 >> 2);
#pragma unroll
        for (int i = 0; i < DT; ++i) voff[i] = r * (2 * D) + ((i ^ pp_v_sw<D>(r)) << 6) + 32 * (ql >> 4) + 8 * (l15 & 3);
    }

    if (nt > 0) {
        load_pages(0);
        load_kv();
        if (nt > 1) load_pages(1);
        store_kv(0);
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) asm volatile("" ::"v"(qf[ks].x), "v"(qf[ks].y), "v"(qf[ks].z), "v"(qf[ks].w));   // flash_walk: retire_q
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
        const int buf = t & 1, kv0 = t * 64;
        if (t + 1 < nt) {
            load_kv();
            if (t + 2 < nt) load_pages(t + 2);
        }
        if (kv0 <= lim_last) {           // else the tile is above every column of this wave (wave-uniform)
            const char* kb = pp_smem + buf * IMG;
            const char* vb = pp_smem + (2 + buf) * IMG;
            f32x16_fl s0, s1;
#pragma unroll
            for (int r = 0; r < 16; ++r) { s0[r] = 0.f; s1[r] = 0.f; }
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const uint4 a0 = *reinterpret_cast<const uint4*>(kb + pp_k_off<D>(ql, 2 * ks + h));
                const uint4 a1 = *reinterpret_cast<const uint4*>(kb + pp_k_off<D>(32 + ql, 2 * ks + h));
                s0 = mfma32<T>(a0, qf[ks], s0);
                s1 = mfma32<T>(a1, qf[ks], s1);
            }
            // this lane holds kv rows (r & 3) + 8 (r >> 2) + 4 h of each 32-row sub-tile; masked by select, never by arithmetic
            if (kv0 + 63 > lim_first) {  // some column's limit falls inside the tile (covers the ragged end: lim <= ctx - 1)
                const int ll = lim - kv0 - 4 * h;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kvl = (r & 3) + 8 * (r >> 2);
                    s0[r] = kvl <= ll ? s0[r] : -INFINITY;
                    s1[r] = 32 + kvl <= ll ? s1[r] : -INFINITY;
                }
            }
            float mx = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; r += 2) mx = fmaxf(fmaxf(fmaxf(s0[r], s1[r]), fmaxf(s0[r + 1], s1[r + 1])), mx);
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            // deferred rescale (flash_softmax_pv): the reference point moves only when the maximum grew by more than 6, so p <= 64
            const float m_new = (mx > m_run + 6.0f || m_run == -INFINITY) ? fmaxf(m_run, mx) : m_run;
            const float m_use = m_new == -INFINITY ? 0.f : m_new;       // nothing visible so far: p = exp2(-inf) = 0
            const bool moved = __builtin_amdgcn_ballot_w64(m_new != m_run) != 0;
            const float alpha = moved ? __builtin_amdgcn_exp2f(m_run - m_use) : 1.0f;
            float ls = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s0[r] = __builtin_amdgcn_exp2f(s0[r] - m_use);
                s1[r] = __builtin_amdgcn_exp2f(s1[r] - m_use);
                ls += s0[r] + s1[r];
            }
            l_run = l_run * alpha + ls;
            m_run = m_new;
            if (moved) {
#pragma unroll
                for (int i = 0; i < DT; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[i][r] *= alpha;
            }
            // O^T += V^T . P^T: 4 k-steps of 16 keys; element j of the B operand is key 16 s + 8 (j >> 2) + 4 h + (j & 3)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                uint4 pb;
                if (s < 2) {
                    pb = make_uint4(pack16x2<T>(s0[8 * s + 0], s0[8 * s + 1]), pack16x2<T>(s0[8 * s + 2], s0[8 * s + 3]),
                                    pack16x2<T>(s0[8 * s + 4], s0[8 * s + 5]), pack16x2<T>(s0[8 * s + 6], s0[8 * s + 7]));
                } else {
                    pb = make_uint4(pack16x2<T>(s1[8 * (s - 2) + 0], s1[8 * (s - 2) + 1]), pack16x2<T>(s1[8 * (s - 2) + 2], s1[8 * (s - 2) + 3]),
                                    pack16x2<T>(s1[8 * (s - 2) + 4], s1[8 * (s - 2) + 5]), pack16x2<T>(s1[8 * (s - 2) + 6], s1[8 * (s - 2) + 7]));
                }
#pragma unroll
                for (int i = 0; i < DT; ++i) {
                    const pp_v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        (__attribute__((address_space(3))) pp_v4s*)(vb + voff[i] + (16 * s) * (2 * D)));
                    const pp_v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        (__attribute__((address_space(3))) pp_v4s*)(vb + voff[i] + (16 * s + 8) * (2 * D)));
                    const uint2 u0 = __builtin_bit_cast(uint2, lo), u1 = __builtin_bit_cast(uint2, hi);
                    o[i] = mfma32<T>(make_uint4(u0.x, u0.y, u1.x, u1.y), pb, o[i]);
                }
            }
        }
        if (t + 1 < nt) store_kv(buf ^ 1);
        __syncthreads();
    }

    // normalise and store: registers 4 g4 .. 4 g4 + 3 of tile i are dims 32 i + 8 g4 + 4 h .. + 3; a column that saw no key has
    // l = 0 and untouched accumulators and stores zeros
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
    if constexpr (KV::fp8) inv *= kv.v_scale[kvh];
    if (store_ok) {
        T* orow = out + row_off;
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                uint2 x;
                x.x = pack16x2<T>(o[i][4 * g4] * inv, o[i][4 * g4 + 1] * inv);
                x.y = pack16x2<T>(o[i][4 * g4 + 2] * inv, o[i][4 * g4 + 3] * inv);
                *reinterpret_cast<uint2*>(orow + i * 32 + 8 * g4 + 4 * h) = x;
            }
    }
}

template <class T, int D, int G, class KV>
static pgk_status paged_prefill_launch(const void* q, const void* kc, const void* vc, const int32_t* block_tables, const int32_t* context_lens,
                                       const int32_t* cu_seqlens_q, void* out, const PagedPrefillGrid& g, int total_tokens, int num_heads,
                                       int num_kv_heads, int block_size, int max_blocks, float scale, const KV& kv, hipStream_t st) {
    using CT = typename std::conditional<KV::fp8, uint8_t, T>::type;
    constexpr size_t LDS = 4 * (size_t)(64 * D * 2);      // the images hold 16-bit words whatever the pages hold
    int bs_shift = -1;
    if ((block_size & (block_size - 1)) == 0)
        for (bs_shift = 0; (1 << bs_shift) < block_size; ++bs_shift) {}
    return launch_dyn_lds<paged_prefill_kernel<T, D, G, KV>>(dim3(g.x, g.y, g.z), 256, LDS, LDS > 48 * 1024, st, (const T*)q, (const CT*)kc,
                                                             (const CT*)vc, block_tables, context_lens, cu_seqlens_q, (T*)out, total_tokens,
                                                             num_heads, num_kv_heads, block_size, bs_shift, max_blocks,
                                                             scale * 1.4426950408889634f, kv);
}

// the two entry points below, after their argument checks; grid3 is what the entry's host-only plan function returned
template <class KV>
static pgk_status paged_prefill_dispatch(const char* name, const void* q, const void* k_cache, const void* v_cache, const int32_t* block_tables,
                                         const int32_t* context_lens, const int32_t* cu_seqlens_q, void* out, const int* grid3, int total_tokens,
                                         int max_query_len, int num_heads, int num_kv_heads, int head_dim, int block_size, int max_blocks_per_seq,
                                         float scale, pgk_dtype dt, const KV& kv, pgk_stream s) {
    if (!(aligned16(q) && aligned16(k_cache) && aligned16(v_cache) && (reinterpret_cast<uintptr_t>(out) & 7u) == 0))
        return set_error(PGK_ERR_INVALID, "%s: q and the caches must be 16-byte aligned, out 8-byte aligned", name);
    if (max_query_len == 0) return PGK_OK;       // every sequence idle
    if (scale <= 0.f) scale = 1.0f / sqrtf((float)head_dim);
    const PagedPrefillGrid g{grid3[0], grid3[1], grid3[2]};
    const int G = num_heads / num_kv_heads;
    hipStream_t st = resolve_stream(s);
#define PGK_PP(TT, DD, GG)                                                                                                                  \
    if (head_dim == DD && G == GG)                                                                                                          \
        return paged_prefill_launch<TT, DD, GG, KV>(q, k_cache, v_cache, block_tables, context_lens, cu_seqlens_q, out, g, total_tokens,   \
                                                    num_heads, num_kv_heads, block_size, max_blocks_per_seq, scale, kv, st);
#define PGK_PP_T(TT) PGK_PP(TT, 128, 1) PGK_PP(TT, 128, 2) PGK_PP(TT, 128, 4) PGK_PP(TT, 128, 8) PGK_PP(TT, 64, 1) PGK_PP(TT, 64, 2) PGK_PP(TT, 64, 4) PGK_PP(TT, 64, 8)
    if (dt == PGK_BF16) { PGK_PP_T(bf16) } else { PGK_PP_T(f16) }
#undef PGK_PP_T
#undef PGK_PP
    return set_error(PGK_ERR_INVALID, "%s: no kernel for D=%d G=%d", name, head_dim, G);
}

}  // namespace pgk

using namespace pgk;

extern "C" {

const char* pgk_paged_prefill_plan(int num_seqs, int max_query_len, int num_heads, int num_kv_heads, int head_dim, pgk_dtype dt, int* grid3) {
    if (const char* why = paged_prefill_refusal(num_heads, num_kv_heads, head_dim, dt == PGK_BF16 || dt == PGK_F16)) {
        set_error(PGK_ERR_INVALID, "pgk_paged_attention_prefill: %s (Hq=%d, Hkv=%d, D=%d, dtype %d)", why, num_heads, num_kv_heads, head_dim, (int)dt);
        return nullptr;
    }
    if (num_seqs < 1 || num_seqs > PP_MAX_SEQS || max_query_len < 0) {
        set_error(PGK_ERR_INVALID, "pgk_paged_attention_prefill: bad batch (seqs=%d of at most %d, max_query_len=%d)", num_seqs, PP_MAX_SEQS, max_query_len);
        return nullptr;
    }
    if (grid3) {
        const PagedPrefillGrid g = paged_prefill_grid(max_query_len, num_heads, num_kv_heads, num_seqs);
        grid3[0] = g.x; grid3[1] = g.y; grid3[2] = g.z;
    }
    return "paged_prefill_mfma";
}

pgk_status pgk_paged_attention_prefill(const void* q, const void* k_cache, const void* v_cache, const int32_t* block_tables,
                                       const int32_t* context_lens, const int32_t* cu_seqlens_q, void* out, int num_seqs, int total_tokens,
                                       int max_query_len, int num_heads, int num_kv_heads, int head_dim, int block_size,
                                       int max_blocks_per_seq, float scale, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(q && k_cache && v_cache && block_tables && context_lens && cu_seqlens_q && out, "pgk_paged_attention_prefill: null pointer");
    PGK_REQUIRE(total_tokens >= 1 && max_query_len >= 0 && max_query_len <= total_tokens,
                "pgk_paged_attention_prefill: bad token counts (total_tokens=%d, max_query_len=%d)", total_tokens, max_query_len);
    PGK_REQUIRE(block_size >= 1 && max_blocks_per_seq >= 1, "pgk_paged_attention_prefill: bad paging (block_size=%d, max_blocks=%d)", block_size,
                max_blocks_per_seq);
    int grid3[3];
    if (!pgk_paged_prefill_plan(num_seqs, max_query_len, num_heads, num_kv_heads, head_dim, dt, grid3)) return PGK_ERR_INVALID;
    return paged_prefill_dispatch("pgk_paged_attention_prefill", q, k_cache, v_cache, block_tables, context_lens, cu_seqlens_q, out, grid3,
                                  total_tokens, max_query_len, num_heads, num_kv_heads, head_dim, block_size, max_blocks_per_seq, scale, dt,
                                  PagedKV16{}, s);
}

pgk_status pgk_paged_attention_prefill_fp8(const void* q, const void* k_cache, const void* v_cache, const float* k_scale, const float* v_scale,
                                           const int32_t* block_tables, const int32_t* context_lens, const int32_t* cu_seqlens_q, void* out,
                                           int num_seqs, int total_tokens, int max_query_len, int num_heads, int num_kv_heads, int head_dim,
                                           int block_size, int max_blocks_per_seq, float scale, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(q && k_cache && v_cache && k_scale && v_scale && block_tables && context_lens && cu_seqlens_q && out,
                "pgk_paged_attention_prefill_fp8: null pointer");
    PGK_REQUIRE(total_tokens >= 1 && max_query_len >= 0 && max_query_len <= total_tokens,
                "pgk_paged_attention_prefill_fp8: bad token counts (total_tokens=%d, max_query_len=%d)", total_tokens, max_query_len);
    PGK_REQUIRE(block_size >= 1 && max_blocks_per_seq >= 1, "pgk_paged_attention_prefill_fp8: bad paging (block_size=%d, max_blocks=%d)", block_size,
                max_blocks_per_seq);
    int grid3[3];
    if (!pgk_paged_kv_fp8_plan(1, num_seqs, max_query_len, num_heads, num_kv_heads, head_dim, dt, grid3)) return PGK_ERR_INVALID;
    return paged_prefill_dispatch("pgk_paged_attention_prefill_fp8", q, k_cache, v_cache, block_tables, context_lens, cu_seqlens_q, out, grid3,
                                  total_tokens, max_query_len, num_heads, num_kv_heads, head_dim, block_size, max_blocks_per_seq, scale, dt,
                                  PagedKV8{k_scale, v_scale}, s);
}

}  // extern "C"
