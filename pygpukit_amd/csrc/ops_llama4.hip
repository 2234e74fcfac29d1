// Llama-4 attention pieces (reference: native/ops/nn/llama4_kernels.cuh, llama4.inl):
//   pgk_l2norm         y = x * rsqrt(mean(x^2) + eps) over the last dimension, no gamma (Llama4TextL2Norm)
//   pgk_irope_scale_q  Q[s][h][:] *= t(positions[s])                            (the stand-alone temperature scaling)
//   pgk_sdpa_irope     softmax(Q.K^T * t(positions[i]) / sqrt(d) + mask) . V    (mask: kv j <= i + causal_offset)
//   pgk_llama4_qk_norm_cache_write   l2norm(Q) in place, l2norm(K) -> k_cache rows, V -> v_cache rows: one launch
//   pgk_sdpa_irope_fixed_cache       sdpa_irope of ONE query row over cache rows 0 .. pos (split-KV flash-decoding)
// The attention itself is flash_fwd_kernel<T, D, FlashIrope> of ops_flash.hip: the reference runs one block per (head,
// query row) over a kv_len-float score array; here the temperature is one more factor in the Q premultiply of the MFMA
// flash kernel and the mask offset is an argument, so sdpa_irope runs at sdpa_causal's speed.

#include "attn_core.hip.h"

namespace pgk {

// ---- l2norm ----------------------------------------------------------------------------------------------------------
// features 64 / 128 (the model's [S * H, head_dim] case): a row is held by the LANES = features / Vec<T>::N lanes that one
// 16-byte load each covers (8 .. 32), a wave takes 64 / LANES rows, the sum of squares is a DPP reduction inside the group.
// in == out is fine: a lane writes only what it has read.
// f: this lane's N values of a row of F that LANES = F / N consecutive lanes hold together -> the normalised values.
// Every lane of the wave must call it (the sum of squares is a DPP reduction inside the group).
template <int F, int N>
__device__ __forceinline__ void l2norm_row_values(float (&f)[N], float eps) {
    constexpr int LANES = F / N;
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < N; ++j) ss += f[j] * f[j];
    ss = group_sum<LANES>(ss);
    const float inv = 1.0f / sqrtf(ss / F + eps);
#pragma unroll
    for (int j = 0; j < N; ++j) f[j] *= inv;
}

template <class T, int F>
__global__ __launch_bounds__(256) void l2norm_rows_kernel(const T* x, T* out, int rows, float eps) {
    constexpr int N = Vec<T>::N, LANES = F / N;
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long row = gid / LANES;
    const int c = (int)(gid % LANES);
    const bool on = row < rows;               // whole groups: 256 % LANES == 0
    float f[N];
    Vec<T> v;
    v.raw = make_uint4(0, 0, 0, 0);
    if (on) v.load(x + row * F + c * N);
    v.to_float(f);
    l2norm_row_values<F, N>(f, eps);          // every lane of the wave takes part
    v.from_float(f);
    if (on) v.store(out + row * F + c * N);
}

// any other feature count: one 256-thread block per row, scalar accesses
template <class T>
__global__ __launch_bounds__(256) void l2norm_block_kernel(const T* x, T* out, int features, float eps) {
    __shared__ float scratch[16];
    const T* xr = x + (size_t)blockIdx.x * features;
    T* orow = out + (size_t)blockIdx.x * features;
    float ss = 0.f;
    for (int i = threadIdx.x; i < features; i += 256) {
        const float a = to_f(xr[i]);
        ss += a * a;
    }
    const float inv = 1.0f / sqrtf(block_sum(ss, scratch) / features + eps);   // its barriers order the reads above before the writes below
    for (int i = threadIdx.x; i < features; i += 256) orow[i] = from_f<T>(to_f(xr[i]) * inv);
}

template <class T>
static pgk_status launch_l2norm(const void* in, void* out, int rows, int features, float eps, hipStream_t st) {
    const T* x = static_cast<const T*>(in);
    T* o = static_cast<T*>(out);
    if (rows == 0) return PGK_OK;
    if ((features == 64 || features == 128) && aligned16(in) && aligned16(out)) {
        const int lanes = features / Vec<T>::N;
        const unsigned grid = (unsigned)(((long long)rows * lanes + 255) / 256);
        if (features == 128) l2norm_rows_kernel<T, 128><<<grid, 256, 0, st>>>(x, o, rows, eps);
        else l2norm_rows_kernel<T, 64><<<grid, 256, 0, st>>>(x, o, rows, eps);
    } else {
        l2norm_block_kernel<T><<<rows, 256, 0, st>>>(x, o, features, eps);
    }
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

// ---- irope_scale_q ---------------------------------------------------------------------------------------------------
// fp32 multiply, one round-to-nearest-even to T.  VEC: one thread per 16-byte chunk (head_dim % 8 == 0, aligned base).
template <class T, bool VEC>
__global__ __launch_bounds__(256) void irope_scale_q_kernel(const T* q, const void* positions, T* out, long long n_items, int row_items,
                                                            float attn_scale, float floor_scale, int pos_is_i64) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= n_items) return;
    const float t = irope_temperature(irope_position(positions, (int)(gid / row_items), pos_is_i64), attn_scale, floor_scale);
    if constexpr (VEC) {
        Vec<T> v;
        v.load(q + gid * 8);
        float f[8];
        v.to_float(f);
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] *= t;
        v.from_float(f);
        v.store(out + gid * 8);
    } else {
        out[gid] = from_f<T>(to_f(q[gid]) * t);
    }
}

template <class T>
static pgk_status launch_irope_scale_q(const void* q, const void* positions, void* out, int seq_len, int n_heads, int head_dim,
                                       float attn_scale, float floor_scale, int pos_is_i64, hipStream_t st) {
    const long long row = (long long)n_heads * head_dim, total = row * seq_len;
    if (total == 0) return PGK_OK;
    if (head_dim % 8 == 0 && aligned16(q) && aligned16(out)) {
        const long long n = total / 8;
        irope_scale_q_kernel<T, true><<<(unsigned)((n + 255) / 256), 256, 0, st>>>((const T*)q, positions, (T*)out, n, (int)(row / 8),
                                                                                  attn_scale, floor_scale, pos_is_i64);
    } else {
        irope_scale_q_kernel<T, false><<<(unsigned)((total + 255) / 256), 256, 0, st>>>((const T*)q, positions, (T*)out, total, (int)row,
                                                                                       attn_scale, floor_scale, pos_is_i64);
    }
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

// ---- llama4_qk_norm_cache_write --------------------------------------------------------------------------------------
// One lane-group (D / 8 lanes, a 16-byte access each) per head row of the S x (Hq + 2 Hkv) head rows of q | k | v:
//   Q head  : normalised in place                                   (l2norm_rows_kernel's arithmetic: l2norm_row_values)
//   K head  : normalised, written to k_cache[h][pos0 + s]            (k itself is left as projected)
//   V head  : copied to v_cache[h][pos0 + s]
// A row pos0 + s outside [0, max_seq) is not written (a device-resident position is not checked by the host).
template <class T, int D>
__global__ __launch_bounds__(256) void qk_norm_cache_write_kernel(T* q, const T* k, const T* v, T* k_cache, T* v_cache, int seq, int hq,
                                                                  int hkv, int max_seq, float eps, int qk_norm, int host_pos,
                                                                  const int32_t* pos_buf) {
    constexpr int N = Vec<T>::N, LANES = D / N;
    const int per_row = hq + 2 * hkv;
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long item = gid / LANES;
    const int c = (int)(gid % LANES);
    const bool on = item < (long long)seq * per_row;      // whole groups: 256 % LANES == 0
    const int s = on ? (int)(item / per_row) : 0, j = on ? (int)(item % per_row) : 0;
    const bool is_q = j < hq, is_k = !is_q && j < hq + hkv;
    const int h = is_q ? j : (is_k ? j - hq : j - hq - hkv);
    const T* src = is_q ? q + ((size_t)s * hq + h) * D : (is_k ? k : v) + ((size_t)s * hkv + h) * D;
    Vec<T> x;
    x.raw = make_uint4(0, 0, 0, 0);
    if (on) x.load(src + c * N);
    float f[N];
    x.to_float(f);
    l2norm_row_values<D, N>(f, eps);                      // every lane of the wave takes part, V rows and idle lanes too
    if (qk_norm && (is_q || is_k)) x.from_float(f);       // V rows, and everything without qk_norm, keep their bits
    if (!on) return;
    if (is_q) {
        if (qk_norm) x.store(q + ((size_t)s * hq + h) * D + c * N);
        return;
    }
    const long long row = (long long)(pos_buf ? pos_buf[0] : host_pos) + s;
    if (row < 0 || row >= max_seq) return;                // never write outside the cache
    x.store((is_k ? k_cache : v_cache) + ((size_t)h * max_seq + (size_t)row) * D + c * N);
}

}  // namespace pgk

using namespace pgk;

extern "C" {

pgk_status pgk_l2norm(const void* in, void* out, int rows, int features, float eps, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(in && out, "pgk_l2norm: null pointer");
    PGK_REQUIRE(rows >= 0 && features >= 1, "pgk_l2norm: bad shape [%d,%d]", rows, features);
    hipStream_t st = resolve_stream(s);
    PGK_DISPATCH_FLOAT(dt, "pgk_l2norm", return (launch_l2norm<T>(in, out, rows, features, eps, st)));
    return PGK_OK;
}

pgk_status pgk_irope_scale_q(const void* q, const void* positions, void* out, int seq_len, int n_heads, int head_dim,
                             float attn_scale, float floor_scale, pgk_dtype pos_dt, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(q && positions && out, "pgk_irope_scale_q: null pointer");
    PGK_REQUIRE(seq_len >= 0 && n_heads >= 1 && head_dim >= 1, "pgk_irope_scale_q: bad shape [%d,%d,%d]", seq_len, n_heads, head_dim);
    PGK_REQUIRE((long long)seq_len * n_heads * head_dim / 8 < (1LL << 31), "pgk_irope_scale_q: Q too large");
    PGK_REQUIRE(pos_dt == PGK_I64 || pos_dt == PGK_I32, "pgk_irope_scale_q: positions must be int64 or int32 (dtype %d)", (int)pos_dt);
    PGK_REQUIRE(dt == PGK_BF16 || dt == PGK_F16, "pgk_irope_scale_q: float16 / bfloat16 only (dtype %d)", (int)dt);
    PGK_REQUIRE(floor_scale > 0.f, "pgk_irope_scale_q: floor_scale must be positive");
    hipStream_t st = resolve_stream(s);
    const int p64 = pos_dt == PGK_I64;
    if (dt == PGK_BF16) return launch_irope_scale_q<bf16>(q, positions, out, seq_len, n_heads, head_dim, attn_scale, floor_scale, p64, st);
    return launch_irope_scale_q<f16>(q, positions, out, seq_len, n_heads, head_dim, attn_scale, floor_scale, p64, st);
}

pgk_status pgk_sdpa_irope(const void* q, const void* k, const void* v, const void* positions, void* out, int hq, int hkv, int q_len,
                          int kv_len, int d, float attn_scale, float floor_scale, int causal_offset, int64_t q_stride_h,
                          int64_t q_stride_s, int64_t kv_stride_h, int64_t kv_stride_s, int64_t o_stride_h, int64_t o_stride_s,
                          pgk_dtype pos_dt, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(q && k && v && positions && out, "pgk_sdpa_irope: null pointer");
    PGK_REQUIRE(dt == PGK_BF16 || dt == PGK_F16, "pgk_sdpa_irope: float16 / bfloat16 only (dtype %d)", (int)dt);
    PGK_REQUIRE(d == 64 || d == 128, "pgk_sdpa_irope: head_dim must be 64 or 128 (got %d)", d);
    PGK_REQUIRE(hq > 0 && hkv > 0 && hq % hkv == 0, "pgk_sdpa_irope: n_heads mismatch (Hq=%d, Hkv=%d)", hq, hkv);
    PGK_REQUIRE(q_len >= 1 && kv_len >= 1, "pgk_sdpa_irope: bad shape q_len=%d kv_len=%d", q_len, kv_len);
    PGK_REQUIRE(causal_offset >= 0, "pgk_sdpa_irope: causal_offset must be >= 0 (got %d): row 0 would see no key", causal_offset);
    PGK_REQUIRE(pos_dt == PGK_I64 || pos_dt == PGK_I32, "pgk_sdpa_irope: positions must be int64 or int32 (dtype %d)", (int)pos_dt);
    PGK_REQUIRE(floor_scale > 0.f, "pgk_sdpa_irope: floor_scale must be positive");
    PGK_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out) &&
                    ((q_stride_h | q_stride_s | kv_stride_h | kv_stride_s | o_stride_h | o_stride_s) & 7) == 0,
                "pgk_sdpa_irope: pointers must be 16-byte aligned and strides multiples of 8 elements");
    PGK_REQUIRE(q_stride_h >= 0 && q_stride_s >= 0 && kv_stride_h >= 0 && kv_stride_s >= 0 && o_stride_h >= 0 && o_stride_s >= 0,
                "pgk_sdpa_irope: negative stride");
    const FlashStrides sd{q_stride_h, q_stride_s, kv_stride_h, kv_stride_s, o_stride_h, o_stride_s};
    return flash_prefill_irope(q, k, v, positions, out, hq, hkv, q_len, kv_len, d, attn_scale, floor_scale, causal_offset, sd,
                               pos_dt == PGK_I64, dt == PGK_BF16 ? 0 : 1, resolve_stream(s));
}

pgk_status pgk_llama4_qk_norm_cache_write(void* q, const void* k, const void* v, void* k_cache, void* v_cache, int seq, int hq, int hkv,
                                          int max_seq, int d, float eps, int qk_norm, int h_pos, const int32_t* pos_buf, pgk_dtype dt,
                                          pgk_stream s) {
    PGK_REQUIRE(q && k && v && k_cache && v_cache, "pgk_llama4_qk_norm_cache_write: null pointer");
    PGK_REQUIRE(dt == PGK_BF16 || dt == PGK_F16, "pgk_llama4_qk_norm_cache_write: float16 / bfloat16 only (dtype %d)", (int)dt);
    PGK_REQUIRE(d == 64 || d == 128, "pgk_llama4_qk_norm_cache_write: head_dim must be 64 or 128 (got %d)", d);
    PGK_REQUIRE(hq > 0 && hkv > 0 && hq % hkv == 0, "pgk_llama4_qk_norm_cache_write: n_heads mismatch (Hq=%d, Hkv=%d)", hq, hkv);
    PGK_REQUIRE(seq >= 1 && max_seq >= 1, "pgk_llama4_qk_norm_cache_write: bad shape seq=%d max_seq=%d", seq, max_seq);
    PGK_REQUIRE(pos_buf || (h_pos >= 0 && (long long)h_pos + seq <= max_seq), "pgk_llama4_qk_norm_cache_write: rows %d..%lld outside cache of %d",
                h_pos, (long long)h_pos + seq, max_seq);
    PGK_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(k_cache) && aligned16(v_cache),
                "pgk_llama4_qk_norm_cache_write: pointers must be 16-byte aligned");
    const long long lanes = (long long)seq * (hq + 2 * hkv) * (d / 8);
    PGK_REQUIRE((lanes + 255) / 256 < (1LL << 31), "pgk_llama4_qk_norm_cache_write: too many rows");
    hipStream_t st = resolve_stream(s);
    const unsigned grid = (unsigned)((lanes + 255) / 256);
#define PGK_PREP(T, DD)                                                                                                                  \
    qk_norm_cache_write_kernel<T, DD><<<grid, 256, 0, st>>>((T*)q, (const T*)k, (const T*)v, (T*)k_cache, (T*)v_cache, seq, hq, hkv, max_seq, \
                                                            eps, qk_norm, h_pos, pos_buf)
    if (dt == PGK_BF16) { if (d == 128) PGK_PREP(bf16, 128); else PGK_PREP(bf16, 64); }
    else { if (d == 128) PGK_PREP(f16, 128); else PGK_PREP(f16, 64); }
#undef PGK_PREP
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

pgk_status pgk_sdpa_irope_fixed_cache(const void* q, const void* k_cache, const void* v_cache, void* out, int hq, int hkv, int max_seq,
                                      int d, float attn_scale, float floor_scale, int h_pos, const int32_t* pos_buf, void* workspace,
                                      pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(q && k_cache && v_cache && out && workspace, "pgk_sdpa_irope_fixed_cache: null pointer");
    PGK_REQUIRE(dt == PGK_BF16 || dt == PGK_F16, "pgk_sdpa_irope_fixed_cache: float16 / bfloat16 only (dtype %d)", (int)dt);
    PGK_REQUIRE(d == 64 || d == 128, "pgk_sdpa_irope_fixed_cache: head_dim must be 64 or 128 (got %d)", d);
    PGK_REQUIRE(hq > 0 && hkv > 0 && hq % hkv == 0, "pgk_sdpa_irope_fixed_cache: n_heads mismatch (Hq=%d, Hkv=%d)", hq, hkv);
    PGK_REQUIRE(max_seq >= 1, "pgk_sdpa_irope_fixed_cache: max_seq=%d", max_seq);
    PGK_REQUIRE(pos_buf || (h_pos >= 0 && h_pos < max_seq), "pgk_sdpa_irope_fixed_cache: position %d outside cache of %d rows", h_pos, max_seq);
    PGK_REQUIRE(floor_scale > 0.f, "pgk_sdpa_irope_fixed_cache: floor_scale must be positive");
    PGK_REQUIRE(aligned16(q) && aligned16(k_cache) && aligned16(v_cache), "pgk_sdpa_irope_fixed_cache: pointers must be 16-byte aligned");
    hipStream_t st = resolve_stream(s);
    const DecodeIrope ex{h_pos, pos_buf, 1.0f / sqrtf((float)d), attn_scale, floor_scale};
    return launch_split_decode16(dt, d, q, k_cache, v_cache, out, workspace, hq, hkv, max_seq, ex, resolve_stream(s));
}

}  // extern "C"
