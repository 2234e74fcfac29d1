// Attention with a clamped relative-position bias table (T5's bucketed bias, one entry per key - query distance):
//   out[h, i] = softmax_j(scale * q[h, i] . k[h / rep, j] + table[h][clamp(j - i, -R, R) + R]) . v[h / rep],   no mask
//   pgk_sdpa_relbias   bf16 / f16 at head_dim 64 / 128 on aligned buffers: flash_fwd_kernel<.., FlashRelBias> (ops_flash.hip);
//                      float32, other head dims up to 256, unaligned buffers, radius > FL_RELBIAS_MAX_RADIUS: the rows kernel below
//   pgk_relbias_plan   which of the two a call takes
// The rows kernel is a correctness path - one wave per (head, query row), fp32 arithmetic, online softmax over chunks of 64 keys -
// and is not tuned.

#include <type_traits>

#include "attn_plan.h"
#include "pgk_device.hip.h"

namespace pgk {

// lane l scores key p0 + l of the chunk; the chunk's probabilities go through LDS so that every lane can weigh its output dims
// (l, l + 64, l + 128, l + 192) with all of them
template <class T>
__global__ __launch_bounds__(64) void relbias_rows_kernel(const T* q, const T* k, const T* v, const float* table, T* out, int hq, int hkv,
                                                          int kv_len, int d, int radius, float scale, FlashStrides sd) {
    __shared__ float qs[RELBIAS_ROWS_MAX_D];
    __shared__ float ps[64];
    const int qi = blockIdx.x, head = blockIdx.y, kvh = head / (hq / hkv), lane = threadIdx.x;
    const T* qr = q + (size_t)head * sd.qh + (size_t)qi * sd.qs;
    for (int j = lane; j < d; j += 64) qs[j] = to_f(qr[j]) * scale;
    __syncthreads();
    const float* trow = table + (size_t)head * (2 * radius + 1) + radius;    // trow[delta], delta in [-radius, radius]
    const T* kb = k + (size_t)kvh * sd.kh;
    const T* vb = v + (size_t)kvh * sd.kh;
    float m = -INFINITY, l = 0.f, acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int p0 = 0; p0 < kv_len; p0 += 64) {
        const int p = p0 + lane;
        float s = -INFINITY;
        if (p < kv_len) {
            const T* kr = kb + (size_t)p * sd.ks;
            float dot = 0.f;
            for (int j = 0; j < d; ++j) dot = fmaf(qs[j], to_f(kr[j]), dot);
            s = dot + trow[min(max(p - qi, -radius), radius)];
        }
        const float m_new = fmaxf(m, wave_max(s));           // finite: the chunk holds at least one key
        const float alpha = expf(m - m_new);                 // first chunk: exp(-inf) = 0 on zero accumulators
        const float e = p < kv_len ? expf(s - m_new) : 0.f;
        l = l * alpha + wave_sum(e);
        m = m_new;
        ps[lane] = e;
        __syncthreads();
        const int n = min(64, kv_len - p0);
#pragma unroll
        for (int a = 0; a < 4; ++a) acc[a] *= alpha;
        for (int i = 0; i < n; ++i) {
            const float pe = ps[i];
            const T* vr = vb + (size_t)(p0 + i) * sd.ks;
#pragma unroll
            for (int a = 0; a < 4; ++a)
                if (lane + 64 * a < d) acc[a] = fmaf(pe, to_f(vr[lane + 64 * a]), acc[a]);
        }
        __syncthreads();
    }
    const float inv = 1.f / l;      // l >= 1: the row's largest score contributes exp(0)
    T* orow = out + (size_t)head * sd.oh + (size_t)qi * sd.os;
#pragma unroll
    for (int a = 0; a < 4; ++a)
        if (lane + 64 * a < d) orow[lane + 64 * a] = from_f<T>(acc[a] * inv);
}

static const char* relbias_leaf(SdpaKernel pick) { return pick == SDPA_FLASH2 ? "relbias_flash" : "relbias_rows"; }

template <class T>
static pgk_status relbias_dispatch(const void* q, const void* k, const void* v, const float* table, void* out, int hq, int hkv, int q_len,
                                   int kv_len, int d, int radius, float scale, const FlashStrides& sd, hipStream_t st) {
    constexpr bool HALF = !std::is_same<T, float>::value;
    const bool in16 = aligned16(q) && aligned16(k) && aligned16(v), out8 = (reinterpret_cast<uintptr_t>(out) & 7u) == 0;
    const SdpaKernel pick = relbias_pick(HALF, d, radius, in16, out8, sd, sdpa_flash_enabled());
    if constexpr (HALF) {
        if (pick == SDPA_FLASH2)
            return flash_prefill_relbias(q, k, v, table, out, hq, hkv, q_len, kv_len, d, radius, scale, sd, std::is_same<T, f16>::value ? 1 : 0,
                                         st);
    }
    if (d > RELBIAS_ROWS_MAX_D) return set_error(PGK_ERR_UNSUPPORTED, "pgk_sdpa_relbias: the rows kernel supports head_dim <= %d (got %d)", RELBIAS_ROWS_MAX_D, d);
    if (hq > 65535) return set_error(PGK_ERR_UNSUPPORTED, "pgk_sdpa_relbias: the rows kernel supports up to 65535 heads (got %d)", hq);
    relbias_rows_kernel<T><<<dim3(q_len, hq), 64, 0, st>>>((const T*)q, (const T*)k, (const T*)v, table, (T*)out, hq, hkv, kv_len, d, radius, scale,
                                                           sd);
    PGK_CHECK_HIP(hipGetLastError());
    return PGK_OK;
}

}  // namespace pgk

using namespace pgk;

extern "C" {

pgk_status pgk_sdpa_relbias(const void* q, const void* k, const void* v, const void* table, void* out, int hq, int hkv, int q_len, int kv_len,
                            int d, int radius, float scale, int64_t q_stride_h, int64_t q_stride_s, int64_t kv_stride_h, int64_t kv_stride_s,
                            int64_t o_stride_h, int64_t o_stride_s, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(q && k && v && table && out, "pgk_sdpa_relbias: null pointer");
    PGK_REQUIRE(hq > 0 && hkv > 0 && hq % hkv == 0, "pgk_sdpa_relbias: n_heads mismatch (Hq=%d, Hkv=%d)", hq, hkv);
    PGK_REQUIRE(q_len > 0 && kv_len > 0 && d > 0, "pgk_sdpa_relbias: bad shape q_len=%d kv_len=%d D=%d", q_len, kv_len, d);
    PGK_REQUIRE(radius >= 0 && radius < (1 << 24), "pgk_sdpa_relbias: radius %d outside [0, 2^24)", radius);
    PGK_REQUIRE((reinterpret_cast<uintptr_t>(table) & 3u) == 0, "pgk_sdpa_relbias: table must be 4-byte aligned");
    PGK_REQUIRE(q_stride_h >= 0 && q_stride_s >= 0 && kv_stride_h >= 0 && kv_stride_s >= 0 && o_stride_h >= 0 && o_stride_s >= 0,
                "pgk_sdpa_relbias: negative stride");
    if (scale <= 0.f) scale = 1.0f / sqrtf((float)d);
    const FlashStrides sd{q_stride_h, q_stride_s, kv_stride_h, kv_stride_s, o_stride_h, o_stride_s};
    hipStream_t st = resolve_stream(s);
    PGK_DISPATCH_FLOAT(dt, "pgk_sdpa_relbias",
                       return (relbias_dispatch<T>(q, k, v, (const float*)table, out, hq, hkv, q_len, kv_len, d, radius, scale, sd, st)));
    return PGK_OK;
}

const char* pgk_relbias_plan(int head_dim, int radius, pgk_dtype dt, int aligned) {
    if (head_dim <= 0 || head_dim > RELBIAS_ROWS_MAX_D || radius < 0 || !is_float_dtype(dt)) {
        set_error(PGK_ERR_INVALID, "pgk_relbias_plan: head_dim %d must be within 1..%d, radius %d non-negative, dtype %d a float type", head_dim,
                  RELBIAS_ROWS_MAX_D, radius, (int)dt);
        return nullptr;
    }
    // aligned: q / k / v on 16 bytes, out on 8, strides multiples of 8 elements - a contiguous [H, S, D] call
    const FlashStrides sd{8, 8, 8, 8, 8, 8};
    return relbias_leaf(relbias_pick(dt != PGK_F32, head_dim, radius, aligned != 0, aligned != 0, sd, sdpa_flash_enabled()));
}

}  // extern "C"
