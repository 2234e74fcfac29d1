// Positional-encoding ops beside RoPE (reference: src/pygpukit/ops/nn/rope.py:386-653 -> native/ops/nn/rope_ext_kernels.cuh):
//   pgk_pope_inplace            q, k [S, H, D] += encoding[start_pos + s, :]        (additive sinusoidal encoding)
//   pgk_alibi_compute_bias      bias [H, S, S] = -slope[h] * (i - j), -1e9 above the diagonal when causal
//   pgk_alibi_add_bias          scores [B, H, q_len, kv_len] -= slope[h] * (start_pos + i - j)
//   pgk_sdpa_alibi              causal attention with the ALiBi bias inside the flash kernel (flash_fwd_kernel<.., FlashAlibi>)
//   pgk_sdpa_alibi_fixed_cache  the same over a fixed KV cache: split-KV flash-decoding for one row, the flash kernel for more
// The tables themselves (rope_init_*, pope_init_encoding, alibi_init_slopes) are built on the host (ops/nn/rope.py).
// The reference materialises the bias ([H, S, S] fp32) or adds it to materialised scores; attention here never has the
// scores in memory, so the bias is computed where they live: in the MFMA accumulators (prefill) and on the reduced score
// of a cache row (decode).

#include "attn_core.hip.h"
#include "flash_common.hip.h"

namespace pgk {

int decode_nsplit(int max_seq);         // ops_attention.hip: the split count pgk_sdpa_decode_workspace_bytes sizes for

pgk_status flash_prefill_alibi(const void* q, const void* k, const void* v, const float* slopes, void* out, int hq, int hkv, int q_len,
                               int kv_len, int d, float scale, long long qh, long long qs, long long kh, long long ks, long long oh,
                               long long os, int dt16, hipStream_t st);

// ---- pope_inplace ----------------------------------------------------------------------------------------------------
// x = round(float(x) + enc[start_pos + s][d]): one fp32 add, one round-to-nearest-even to T.  One launch covers q (the first
// nq items) and k.  VEC: one thread per 16-byte chunk of q / k (head_dim % 8 == 0, aligned bases), else one per element.
template <class T, bool VEC>
__global__ __launch_bounds__(256) void pope_inplace_kernel(T* q, T* k, const float* enc, long long nq, long long nk, int q_row, int k_row,
                                                           int d, int start_pos) {
    constexpr int N = VEC ? Vec<T>::N : 1;
    long long item = (long long)blockIdx.x * 256 + threadIdx.x;
    if (item >= nq + nk) return;
    T* x = q;
    int row = q_row;                          // elements of one position: heads * head_dim
    if (item >= nq) { item -= nq; x = k; row = k_row; }
    const long long e = item * N;
    const float* er = enc + ((long long)start_pos + e / row) * d + (int)(e % d);
    if constexpr (VEC) {
        Vec<T> v;
        v.load(x + e);
        float f[N];
        v.to_float(f);
#pragma unroll
        for (int j = 0; j < N; j += 4) {
            const float4 a = *reinterpret_cast<const float4*>(er + j);
            f[j] += a.x; f[j + 1] += a.y; f[j + 2] += a.z; f[j + 3] += a.w;
        }
        v.from_float(f);
        v.store(x + e);
    } else {
        x[e] = from_f<T>(to_f(x[e]) + er[0]);
    }
}

template <class T>
static pgk_status launch_pope(void* q, void* k, const void* enc, int seq, int hq, int hk, int d, int start_pos, hipStream_t st) {
    const long long tq = (long long)seq * hq * d, tk = (long long)seq * hk * d;
    if (tq + tk == 0) return PGK_OK;
    const float* e = static_cast<const float*>(enc);
    if (d % 8 == 0 && aligned16(q) && aligned16(k) && aligned16(enc)) {
        constexpr int N = Vec<T>::N;
        const long long n = (tq + tk) / N;
        pope_inplace_kernel<T, true><<<(unsigned)((n + 255) / 256), 256, 0, st>>>((T*)q, (T*)k, e, tq / N, tk / N, hq * d, hk * d, d, start_pos);
    } else {
        pope_inplace_kernel<T, false><<<(unsigned)((tq + tk + 255) / 256), 256, 0, st>>>((T*)q, (T*)k, e, tq, tk, hq * d, hk * d, d, start_pos);
    }
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

// ---- alibi_compute_bias / alibi_add_bias -----------------------------------------------------------------------------
// One fp32 multiply per element: (i - j) is an exact fp32 integer.
__global__ __launch_bounds__(256) void alibi_bias_kernel(const float* slopes, float* bias, long long total, int seq, int causal) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    const int j = (int)(gid % seq), i = (int)(gid / seq % seq), h = (int)(gid / seq / seq);
    bias[gid] = (causal && j > i) ? -1e9f : -slopes[h] * (float)(i - j);
}

// Product and difference are rounded separately, as the host computes them: contraction is off for this body (hipcc fuses
// a * b - c into an FMA by default, through __fmul_rn / __fsub_rn as well - they are plain operators in HIP).
__global__ __launch_bounds__(256) void alibi_add_bias_kernel(float* scores, const float* slopes, long long total, int heads, int q_len,
                                                             int kv_len, int start_pos) {
#pragma clang fp contract(off)
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    const int j = (int)(gid % kv_len), i = (int)(gid / kv_len % q_len), h = (int)(gid / kv_len / q_len % heads);
    const float prod = slopes[h] * (float)(start_pos + i - j);
    scores[gid] = scores[gid] - prod;
}

// ---- sdpa_alibi_fixed_cache, q_len == 1 ------------------------------------------------------------------------------
// decode_phase1_kernel of ops_attention.hip with -slope[head] * (ctx - 1 - pos) added in fp32 to the score of cache row pos
// before the online softmax.  Same chunking, records and phase 2 as pgk_sdpa_fixed_cache.
template <int G>
struct AlibiDecodeBias {
    float slope[G];
    int last;                                       // the query's position: context_len - 1
    __device__ __forceinline__ float operator()(int g, int pos) const { return -slope[g] * (float)(last - pos); }
};

template <class T, int D, int G>
__global__ __launch_bounds__(256) void alibi_decode_phase1_kernel(const T* q, const T* kc, const T* vc, const float* slopes, float* ws,
                                                                  int hq, int hkv, int max_seq, float scale, int host_ctx,
                                                                  const int32_t* ctx_buf, int nsplit) {
    constexpr int LPR = D / 8, PPW = 64 / LPR, RS = D + 2;
    __shared__ float lds[4 * PPW * G * RS];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int ctx = max(min(ctx_buf ? ctx_buf[0] : host_ctx, max_seq), 0);
    const int h0 = blockIdx.y * G;                  // G consecutive query heads of one kv head (G divides Hq / Hkv)
    const int kv_head = h0 / (hq / hkv);
    const int chunk = decode_chunk_len(ctx, nsplit);
    const int c0 = min(blockIdx.x * chunk, ctx), c1 = min(c0 + chunk, ctx);
    float qf[G][8];
    AlibiDecodeBias<G> bias;
    bias.last = ctx - 1;
    const int sub = lane % LPR;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        KVLoad<T>::load8(q + (size_t)(h0 + g) * D + sub * 8, qf[g]);
#pragma unroll
        for (int j = 0; j < 8; ++j) qf[g][j] *= scale;
        bias.slope[g] = slopes[h0 + g];
    }
    DecodeState<G> st;
    st.init();
    decode_walk<T, D, G>(kc + (size_t)kv_head * max_seq * D, vc + (size_t)kv_head * max_seq * D, c0, c1, qf, lane, wid, st, bias);
    decode_block_merge<D, G>(st, lds, ws + ((size_t)h0 * nsplit + blockIdx.x) * RS, (size_t)nsplit * RS, lane, wid);
}

template <class T, int D>
static pgk_status launch_alibi_decode(const void* q, const void* kc, const void* vc, const float* slopes, void* out, float* ws, int hq,
                                      int hkv, int max_seq, float scale, int host_ctx, const int32_t* ctx_buf, hipStream_t st) {
    const int nsplit = decode_nsplit(max_seq), rep = hq / hkv;
    // head grouping as pgk_sdpa_irope_fixed_cache (ops_llama4.hip, where the five-head case was measured)
    int G = rep % 4 == 0 ? 4 : rep % 2 == 0 ? 2 : 1;
    if (G == 1 && rep % 5 == 0 && (long long)nsplit * (hq / 5) >= 256) G = 5;
    const dim3 grid(nsplit, hq / G);
#define PGK_ALIBI_DEC(GG)                                                                                                                 \
    case GG:                                                                                                                              \
        alibi_decode_phase1_kernel<T, D, GG><<<grid, 256, 0, st>>>((const T*)q, (const T*)kc, (const T*)vc, slopes, ws, hq, hkv, max_seq, \
                                                                   scale, host_ctx, ctx_buf, nsplit);                                     \
        break;
    switch (G) { PGK_ALIBI_DEC(1) PGK_ALIBI_DEC(2) PGK_ALIBI_DEC(4) PGK_ALIBI_DEC(5) }
#undef PGK_ALIBI_DEC
    decode_phase2_kernel<T, D><<<hq, D, 0, st>>>(ws, (T*)out, nsplit);
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

}  // namespace pgk

using namespace pgk;

extern "C" {

pgk_status pgk_pope_inplace(void* q, void* k, const void* encoding, int seq, int hq, int hk, int d, int start_pos, int max_seq,
                            pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(q && k && encoding, "pgk_pope_inplace: null pointer");
    PGK_REQUIRE(seq >= 0 && hq >= 1 && hk >= 1 && d >= 1 && max_seq >= 1, "pgk_pope_inplace: bad shape seq=%d hq=%d hk=%d d=%d max_seq=%d", seq,
                hq, hk, d, max_seq);
    PGK_REQUIRE(start_pos >= 0 && (long long)start_pos + seq <= max_seq, "pgk_pope_inplace: rows %d..%lld outside the encoding table of %d rows",
                start_pos, (long long)start_pos + seq, max_seq);
    PGK_REQUIRE((long long)seq * (hq + hk) * d / 256 < (1LL << 31) - 1, "pgk_pope_inplace: q / k too large");
    hipStream_t st = resolve_stream(s);
    PGK_DISPATCH_FLOAT(dt, "pgk_pope_inplace", return (launch_pope<T>(q, k, encoding, seq, hq, hk, d, start_pos, st)));
    return PGK_OK;
}

pgk_status pgk_alibi_compute_bias(const void* slopes, void* bias, int seq_len, int num_heads, int causal, pgk_stream s) {
    PGK_REQUIRE(slopes && bias, "pgk_alibi_compute_bias: null pointer");
    PGK_REQUIRE(seq_len >= 1 && num_heads >= 1, "pgk_alibi_compute_bias: bad shape seq_len=%d num_heads=%d", seq_len, num_heads);
    const long long total = (long long)num_heads * seq_len * seq_len;
    PGK_REQUIRE(total / 256 < (1LL << 31) - 1, "pgk_alibi_compute_bias: bias too large");
    alibi_bias_kernel<<<(unsigned)((total + 255) / 256), 256, 0, resolve_stream(s)>>>((const float*)slopes, (float*)bias, total, seq_len, causal);
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

pgk_status pgk_alibi_add_bias(void* scores, const void* slopes, int batch, int num_heads, int q_len, int kv_len, int start_pos,
                              pgk_dtype scores_dt, pgk_dtype slopes_dt, int n_slopes, pgk_stream s) {
    PGK_REQUIRE(scores && slopes, "pgk_alibi_add_bias: null pointer");
    PGK_REQUIRE(scores_dt == PGK_F32 && slopes_dt == PGK_F32, "pgk_alibi_add_bias: scores and slopes must be float32 (dtypes %d, %d)",
                (int)scores_dt, (int)slopes_dt);
    PGK_REQUIRE(batch >= 0 && num_heads >= 1 && q_len >= 0 && kv_len >= 0, "pgk_alibi_add_bias: bad shape [%d,%d,%d,%d]", batch, num_heads, q_len,
                kv_len);
    PGK_REQUIRE(n_slopes == num_heads, "pgk_alibi_add_bias: %d slopes for %d heads", n_slopes, num_heads);
    const long long total = (long long)batch * num_heads * q_len * kv_len;
    PGK_REQUIRE(total / 256 < (1LL << 31) - 1, "pgk_alibi_add_bias: scores too large");
    if (total == 0) return PGK_OK;
    alibi_add_bias_kernel<<<(unsigned)((total + 255) / 256), 256, 0, resolve_stream(s)>>>((float*)scores, (const float*)slopes, total, num_heads,
                                                                                         q_len, kv_len, start_pos);
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

pgk_status pgk_sdpa_alibi(const void* q, const void* k, const void* v, const void* slopes, void* out, int hq, int hkv, int q_len, int kv_len,
                          int d, float scale, int64_t q_stride_h, int64_t q_stride_s, int64_t kv_stride_h, int64_t kv_stride_s,
                          int64_t o_stride_h, int64_t o_stride_s, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(q && k && v && slopes && out, "pgk_sdpa_alibi: null pointer");
    PGK_REQUIRE(dt == PGK_BF16 || dt == PGK_F16, "pgk_sdpa_alibi: float16 / bfloat16 only (dtype %d)", (int)dt);
    PGK_REQUIRE(d == 64 || d == 128, "pgk_sdpa_alibi: head_dim must be 64 or 128 (got %d)", d);
    PGK_REQUIRE(hq > 0 && hkv > 0 && hq % hkv == 0, "pgk_sdpa_alibi: n_heads mismatch (Hq=%d, Hkv=%d)", hq, hkv);
    PGK_REQUIRE(q_len >= 1 && kv_len >= q_len, "pgk_sdpa_alibi: needs kv_len >= q_len >= 1 (q_len=%d kv_len=%d)", q_len, kv_len);
    PGK_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out) &&
                    ((q_stride_h | q_stride_s | kv_stride_h | kv_stride_s | o_stride_h | o_stride_s) & 7) == 0,
                "pgk_sdpa_alibi: pointers must be 16-byte aligned and strides multiples of 8 elements");
    PGK_REQUIRE(q_stride_h >= 0 && q_stride_s >= 0 && kv_stride_h >= 0 && kv_stride_s >= 0 && o_stride_h >= 0 && o_stride_s >= 0,
                "pgk_sdpa_alibi: negative stride");
    if (scale <= 0.f) scale = 1.0f / sqrtf((float)d);
    return flash_prefill_alibi(q, k, v, (const float*)slopes, out, hq, hkv, q_len, kv_len, d, scale, q_stride_h, q_stride_s, kv_stride_h,
                               kv_stride_s, o_stride_h, o_stride_s, dt == PGK_BF16 ? 0 : 1, resolve_stream(s));
}

pgk_status pgk_sdpa_alibi_fixed_cache(const void* q, const void* k_cache, const void* v_cache, const void* slopes, void* out, int hq, int hkv,
                                      int q_len, int max_seq, int d, float scale, int h_context_len, const int32_t* ctx_buf, void* workspace,
                                      pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(q && k_cache && v_cache && slopes && out, "pgk_sdpa_alibi_fixed_cache: null pointer");
    PGK_REQUIRE(dt == PGK_BF16 || dt == PGK_F16, "pgk_sdpa_alibi_fixed_cache: float16 / bfloat16 only (dtype %d)", (int)dt);
    PGK_REQUIRE(d == 64 || d == 128, "pgk_sdpa_alibi_fixed_cache: head_dim must be 64 or 128 (got %d)", d);
    PGK_REQUIRE(hq > 0 && hkv > 0 && hq % hkv == 0, "pgk_sdpa_alibi_fixed_cache: n_heads mismatch (Hq=%d, Hkv=%d)", hq, hkv);
    PGK_REQUIRE(q_len >= 1 && max_seq >= 1, "pgk_sdpa_alibi_fixed_cache: bad shape q_len=%d max_seq=%d", q_len, max_seq);
    PGK_REQUIRE(q_len == 1 || !ctx_buf, "pgk_sdpa_alibi_fixed_cache: a device context length requires q_len == 1 (got %d)", q_len);
    PGK_REQUIRE(ctx_buf || (h_context_len >= q_len && h_context_len <= max_seq),
                "pgk_sdpa_alibi_fixed_cache: invalid context_len %d (q_len %d, cache rows %d)", h_context_len, q_len, max_seq);
    PGK_REQUIRE(aligned16(q) && aligned16(k_cache) && aligned16(v_cache) && aligned16(out),
                "pgk_sdpa_alibi_fixed_cache: pointers must be 16-byte aligned");
    if (scale <= 0.f) scale = 1.0f / sqrtf((float)d);
    hipStream_t st = resolve_stream(s);
    const float* sl = (const float*)slopes;
    if (q_len > 1)          // the prefill kernel over the cache in place
        return flash_prefill_alibi(q, k_cache, v_cache, sl, out, hq, hkv, q_len, h_context_len, d, scale, (long long)q_len * d, d,
                                   (long long)max_seq * d, d, (long long)q_len * d, d, dt == PGK_BF16 ? 0 : 1, st);
    PGK_REQUIRE(workspace, "pgk_sdpa_alibi_fixed_cache: q_len == 1 needs a workspace of pgk_sdpa_decode_workspace_bytes");
    float* ws = (float*)workspace;
    if (dt == PGK_BF16) {
        if (d == 128) return launch_alibi_decode<bf16, 128>(q, k_cache, v_cache, sl, out, ws, hq, hkv, max_seq, scale, h_context_len, ctx_buf, st);
        return launch_alibi_decode<bf16, 64>(q, k_cache, v_cache, sl, out, ws, hq, hkv, max_seq, scale, h_context_len, ctx_buf, st);
    }
    if (d == 128) return launch_alibi_decode<f16, 128>(q, k_cache, v_cache, sl, out, ws, hq, hkv, max_seq, scale, h_context_len, ctx_buf, st);
    return launch_alibi_decode<f16, 64>(q, k_cache, v_cache, sl, out, ws, hq, hkv, max_seq, scale, h_context_len, ctx_buf, st);
}

}  // extern "C"
