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

namespace pgk {

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
    const FlashStrides sd{q_stride_h, q_stride_s, kv_stride_h, kv_stride_s, o_stride_h, o_stride_s};
    return flash_prefill_alibi(q, k, v, (const float*)slopes, out, hq, hkv, q_len, kv_len, d, scale, sd, dt == PGK_BF16 ? 0 : 1,
                               resolve_stream(s));
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
    if (q_len > 1) {        // the prefill kernel over the cache in place
        const FlashStrides sd{(long long)q_len * d, d, (long long)max_seq * d, d, (long long)q_len * d, d};
        return flash_prefill_alibi(q, k_cache, v_cache, sl, out, hq, hkv, q_len, h_context_len, d, scale, sd, dt == PGK_BF16 ? 0 : 1, st);
    }
    PGK_REQUIRE(workspace, "pgk_sdpa_alibi_fixed_cache: q_len == 1 needs a workspace of pgk_sdpa_decode_workspace_bytes");
    const DecodeAlibi ex{h_context_len, ctx_buf, scale, sl};
    return launch_split_decode16(dt, d, q, k_cache, v_cache, out, workspace, hq, hkv, max_seq, ex, st);
}

}  // extern "C"
