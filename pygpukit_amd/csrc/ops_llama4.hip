// Llama-4 attention pieces (reference: native/ops/nn/llama4_kernels.cuh, llama4.inl):
//   pgk_l2norm         y = x * rsqrt(mean(x^2) + eps) over the last dimension, no gamma (Llama4TextL2Norm)
//   pgk_irope_scale_q  Q[s][h][:] *= t(positions[s])                            (the stand-alone temperature scaling)
//   pgk_sdpa_irope     softmax(Q.K^T * t(positions[i]) / sqrt(d) + mask) . V    (mask: kv j <= i + causal_offset)
// The attention itself is flash_fwd_kernel<T, D, FlashIrope> of ops_flash.hip: the reference runs one block per (head,
// query row) over a kv_len-float score array; here the temperature is one more factor in the Q premultiply of the MFMA
// flash kernel and the mask offset is an argument, so sdpa_irope runs at sdpa_causal's speed.

#include "flash_common.hip.h"

namespace pgk {

pgk_status flash_prefill_irope(const void* q, const void* k, const void* v, const void* positions, void* out, int hq, int hkv, int q_len,
                               int kv_len, int d, float attn_scale, float floor_scale, int causal_offset, long long qh, long long qs,
                               long long kh, long long ks, long long oh, long long os, int pos_is_i64, int dt16, hipStream_t st);

// ---- l2norm ----------------------------------------------------------------------------------------------------------
// features 64 / 128 (the model's [S * H, head_dim] case): a row is held by the LANES = features / Vec<T>::N lanes that one
// 16-byte load each covers (8 .. 32), a wave takes 64 / LANES rows, the sum of squares is a DPP reduction inside the group.
// in == out is fine: a lane writes only what it has read.
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
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < N; ++j) ss += f[j] * f[j];
    ss = group_sum<LANES>(ss);                // every lane of the wave takes part
    const float inv = 1.0f / sqrtf(ss / F + eps);
#pragma unroll
    for (int j = 0; j < N; ++j) f[j] *= inv;
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
    return flash_prefill_irope(q, k, v, positions, out, hq, hkv, q_len, kv_len, d, attn_scale, floor_scale, causal_offset, q_stride_h,
                               q_stride_s, kv_stride_h, kv_stride_s, o_stride_h, o_stride_s, pos_dt == PGK_I64, dt == PGK_BF16 ? 0 : 1,
                               resolve_stream(s));
}

}  // extern "C"
