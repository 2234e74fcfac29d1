// FP8 (OCP e4m3) KV cache: the quantising cache writer, the per-head absmax scale helper and the split-KV decode over the 8-bit
// cache (attn_kv_fp8.hip.h).  Layout [Hkv][max_seq][D] in uint8, un-expanded only; one fp32 scale per KV head for K and one for V,
// value = e4m3(code) * scale, code = rne_e4m3(clamp(x / scale, +-448)) with x widened to fp32 and a correctly rounded fp32 division.

#include "attn_kv_fp8.hip.h"
#include "pgk_internal.h"

namespace pgk {

// One lane = 16 elements of one row of new_kv [S][Hkv][D]: two 16-byte loads, one 16-byte store to cache row pos + s of head h
// (kv8_quantise16, attn_kv_fp8.hip.h).
template <class T>
__global__ __launch_bounds__(256) void kv8_write_kernel(const T* new_kv, uint8_t* cache, const float* scales, int seq, int hkv, int max_seq,
                                                        int d, int host_pos, const int32_t* pos_buf) {
    const int lpr = d / 16;                                      // lanes per row
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)seq * hkv * lpr) return;
    const int sub = (int)(t % lpr), h = (int)(t / lpr % hkv), s = (int)(t / lpr / hkv);
    const long long row = (long long)(pos_buf ? pos_buf[0] : host_pos) + s;
    if (row < 0 || row >= max_seq) return;                      // a device position outside the cache: not stored (pgk_kv_cache_write's guard)
    const T* src = new_kv + ((size_t)s * hkv + h) * d + sub * 16;
    *reinterpret_cast<uint4*>(cache + ((size_t)h * max_seq + (size_t)row) * d + sub * 16) = kv8_quantise16<T>(src, scales[h]);
}

// One workgroup per KV head: absmax of x[:, h, :] / 224 (half of the e4m3 range is headroom for later tokens), 1 for an all-zero head.
template <class T>
__global__ __launch_bounds__(256) void kv8_absmax_scale_kernel(const T* x, float* scales, int seq, int hkv, int d) {
    __shared__ float red[4];
    const int h = blockIdx.x, vpr = d / 8;                       // 16-byte vectors per row
    float mx = 0.f;
    for (long long i = threadIdx.x; i < (long long)seq * vpr; i += blockDim.x) {
        float f[8];
        KVLoad<T>::load8(x + ((size_t)(i / vpr) * hkv + h) * d + (i % vpr) * 8, f);
#pragma unroll
        for (int j = 0; j < 8; ++j) mx = fmaxf(mx, fabsf(f[j]));
    }
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        scales[h] = mx > 0.f ? __fdiv_rn(mx, 224.f) : 1.f;
    }
}

template <class T, int D>
static pgk_status launch_kv8_decode(const void* q, const void* kc, const void* vc, const float* ks, const float* vs, void* out, void* ws, int hq,
                                    int hkv, int max_seq, float scale, int h_ctx, const int32_t* ctx_buf, hipStream_t st) {
    const int nsplit = decode_nsplit(max_seq), G = decode_heads_per_group(hq, hkv, nsplit, false);
    auto phase1 = [&](auto g) {
        kv8_decode_phase1_kernel<T, D, decltype(g)::value><<<dim3(nsplit, hq / G), 256, 0, st>>>(
            (const T*)q, (const uint8_t*)kc, (const uint8_t*)vc, ks, vs, (float*)ws, hq, hkv, max_seq, nsplit, scale, h_ctx, ctx_buf);
    };
    switch (G) {
        case 1: phase1(std::integral_constant<int, 1>{}); break;
        case 2: phase1(std::integral_constant<int, 2>{}); break;
        default: phase1(std::integral_constant<int, 4>{}); break;
    }
    decode_phase2_kernel<T, D><<<hq, D, 0, st>>>((const float*)ws, (T*)out, nsplit);
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

// what pgk_sdpa_fixed_cache_fp8 needs of a shape: nullptr, or the reason it is rejected
static const char* kv8_reject(int hq, int hkv, int d, int max_seq, pgk_dtype dt, bool aligned) {
    if (hq <= 0 || hkv <= 0 || hq % hkv) return "needs Hq % Hkv == 0";
    if (d != 64 && d != 128) return "head_dim must be 64 or 128";
    if (max_seq < 1) return "cache rows < 1";
    if (dt != PGK_BF16 && dt != PGK_F16) return "q / out must be bfloat16 or float16";
    if (!aligned) return "q and the caches must be 16-byte aligned";
    return nullptr;
}

}  // namespace pgk

using namespace pgk;

extern "C" {

pgk_status pgk_kv_cache_write_fp8(const void* new_kv, void* cache, const float* scales, int seq, int hkv, int max_seq, int d, int h_pos,
                                  const int32_t* pos_buf, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(new_kv && cache && scales, "pgk_kv_cache_write_fp8: null pointer");
    PGK_REQUIRE(hkv > 0 && max_seq > 0 && seq >= 0, "pgk_kv_cache_write_fp8: bad shape seq=%d Hkv=%d rows=%d", seq, hkv, max_seq);
    PGK_REQUIRE(d == 64 || d == 128, "pgk_kv_cache_write_fp8: head_dim must be 64 or 128, got %d", d);
    PGK_REQUIRE(dt == PGK_BF16 || dt == PGK_F16, "pgk_kv_cache_write_fp8: new_kv must be bfloat16 or float16 (dtype %d)", (int)dt);
    PGK_REQUIRE(aligned16(new_kv) && aligned16(cache), "pgk_kv_cache_write_fp8: new_kv and cache must be 16-byte aligned");
    PGK_REQUIRE(pos_buf || (h_pos >= 0 && (long long)h_pos + seq <= max_seq), "pgk_kv_cache_write_fp8: rows %d..%lld outside cache of %d", h_pos,
                (long long)h_pos + seq - 1, max_seq);
    if (seq == 0) return PGK_OK;
    hipStream_t st = resolve_stream(s);
    const long long lanes = (long long)seq * hkv * (d / 16);
    const dim3 grid((unsigned)ceil_div(lanes, 256));
    if (dt == PGK_BF16)
        kv8_write_kernel<bf16><<<grid, 256, 0, st>>>((const bf16*)new_kv, (uint8_t*)cache, scales, seq, hkv, max_seq, d, h_pos, pos_buf);
    else
        kv8_write_kernel<f16><<<grid, 256, 0, st>>>((const f16*)new_kv, (uint8_t*)cache, scales, seq, hkv, max_seq, d, h_pos, pos_buf);
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

pgk_status pgk_kv_fp8_absmax_scales(const void* x, float* scales, int seq, int hkv, int d, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(x && scales, "pgk_kv_fp8_absmax_scales: null pointer");
    PGK_REQUIRE(seq >= 1 && hkv >= 1 && d >= 8 && d % 8 == 0, "pgk_kv_fp8_absmax_scales: bad shape seq=%d Hkv=%d D=%d", seq, hkv, d);
    PGK_REQUIRE(dt == PGK_BF16 || dt == PGK_F16, "pgk_kv_fp8_absmax_scales: x must be bfloat16 or float16 (dtype %d)", (int)dt);
    PGK_REQUIRE(aligned16(x), "pgk_kv_fp8_absmax_scales: x must be 16-byte aligned");
    hipStream_t st = resolve_stream(s);
    if (dt == PGK_BF16) kv8_absmax_scale_kernel<bf16><<<hkv, 256, 0, st>>>((const bf16*)x, scales, seq, hkv, d);
    else kv8_absmax_scale_kernel<f16><<<hkv, 256, 0, st>>>((const f16*)x, scales, seq, hkv, d);
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

pgk_status pgk_sdpa_fixed_cache_fp8(const void* q, const void* k_cache, const void* v_cache, const float* k_scale, const float* v_scale, void* out,
                                    int hq, int hkv, int max_seq, int d, float scale, int h_context_len, const int32_t* ctx_buf, void* workspace,
                                    pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(q && k_cache && v_cache && k_scale && v_scale && out && workspace, "pgk_sdpa_fixed_cache_fp8: null pointer");
    const char* why = kv8_reject(hq, hkv, d, max_seq, dt, aligned16(q) && aligned16(k_cache) && aligned16(v_cache));
    PGK_REQUIRE(!why, "pgk_sdpa_fixed_cache_fp8: %s (heads %d/%d, D %d, rows %d, dtype %d)", why, hq, hkv, d, max_seq, (int)dt);
    PGK_REQUIRE(ctx_buf || (h_context_len > 0 && h_context_len <= max_seq), "pgk_sdpa_fixed_cache_fp8: invalid context_len %d (cache rows %d)",
                h_context_len, max_seq);
    if (scale <= 0.f) scale = 1.0f / sqrtf((float)d);
    hipStream_t st = resolve_stream(s);
    if (dt == PGK_BF16) {
        if (d == 128) return launch_kv8_decode<bf16, 128>(q, k_cache, v_cache, k_scale, v_scale, out, workspace, hq, hkv, max_seq, scale, h_context_len, ctx_buf, st);
        return launch_kv8_decode<bf16, 64>(q, k_cache, v_cache, k_scale, v_scale, out, workspace, hq, hkv, max_seq, scale, h_context_len, ctx_buf, st);
    }
    if (d == 128) return launch_kv8_decode<f16, 128>(q, k_cache, v_cache, k_scale, v_scale, out, workspace, hq, hkv, max_seq, scale, h_context_len, ctx_buf, st);
    return launch_kv8_decode<f16, 64>(q, k_cache, v_cache, k_scale, v_scale, out, workspace, hq, hkv, max_seq, scale, h_context_len, ctx_buf, st);
}

const char* pgk_sdpa_kv_fp8_plan(int hq, int hkv, int d, int max_seq, pgk_dtype dt, int aligned, int* nsplit) {
    if (const char* why = kv8_reject(hq, hkv, d, max_seq, dt, aligned != 0)) {
        set_error(PGK_ERR_INVALID, "pgk_sdpa_kv_fp8_plan: %s (heads %d/%d, D %d, rows %d, dtype %d)", why, hq, hkv, d, max_seq, (int)dt);
        return nullptr;
    }
    if (nsplit) *nsplit = decode_nsplit(max_seq);
    return "kv_fp8_split";
}

}  // extern "C"
