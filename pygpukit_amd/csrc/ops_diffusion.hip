// Diffusion-transformer row kernels: affine-free LayerNorm modulated and gated by per-sample conditioning vectors (AdaLN /
// AdaLN-Zero), fused with the gated residual that precedes it, and the patchify / unpatchify moves.
// One template covers the family (reference: native/ops/nn/diffusion.inl adaln / adaln_zero / layer_norm_simple / modulate /
// gated_residual, five kernels there).  Dispatch as the row norms (ops_norm_rope.hip, base_plan.h): a wave per row with the row
// in registers, else a 256-thread block per row; fp32 math, one rounding per output.  Every multiply-add that reaches an output
// is an explicit fmaf, so the wave and block kernels and the fused and the split forms round alike.

#include "base_plan.h"
#include "pgk_device.hip.h"
#include "pgk_internal.h"

namespace pgk {

struct AdalnArgs {
    const void* x; const void* res; void* sum; void* y;
    const void* gate_tab; const void* gate_vec; const void* scale_tab; const void* scale_vec;
    const void* shift_tab; const void* shift_vec;
    long long gate_stride, scale_stride, shift_stride;   // elements between batch elements of a vector; 0: shared
    int rows, tokens, features, norm;
    float eps;
};

// N consecutive values as fp32: one 16-byte access, or two when the vectors are fp32 under 16-bit rows (N == 8)
template <class VT, int N> __device__ __forceinline__ void load_n(const VT* p, float (&f)[N]) {
    if constexpr (sizeof(VT) * N == 16) {
        Vec<VT> t;
        t.load(p);
        t.to_float(f);
    } else {
        static_assert(sizeof(VT) == 4 && N == 8, "fp32 vectors under 16-bit rows");
        const uint4 lo = *reinterpret_cast<const uint4*>(p), hi = *reinterpret_cast<const uint4*>(p + 4);
        f[0] = __uint_as_float(lo.x); f[1] = __uint_as_float(lo.y); f[2] = __uint_as_float(lo.z); f[3] = __uint_as_float(lo.w);
        f[4] = __uint_as_float(hi.x); f[5] = __uint_as_float(hi.y); f[6] = __uint_as_float(hi.z); f[7] = __uint_as_float(hi.w);
    }
}

// tab[j0 .. j0+N) + vec[j0 .. j0+N), either part optional; `dflt` when both are absent (vec already points at the batch element)
template <class VT, int N>
__device__ __forceinline__ void mod_load(const VT* tab, const VT* vec, int j0, float dflt, float (&f)[N]) {
    if (!tab && !vec) {
#pragma unroll
        for (int j = 0; j < N; ++j) f[j] = dflt;
        return;
    }
    if (tab) {
        load_n<VT, N>(tab + j0, f);
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) f[j] = 0.f;
    }
    if (vec) {
        float g[N];
        load_n<VT, N>(vec + j0, g);
#pragma unroll
        for (int j = 0; j < N; ++j) f[j] += g[j];
    }
}

template <class VT> __device__ __forceinline__ float mod_at(const VT* tab, const VT* vec, int j, float dflt) {
    if (!tab && !vec) return dflt;
    float f = tab ? to_f(tab[j]) : 0.f;
    if (vec) f += to_f(vec[j]);
    return f;
}

template <class VT> __device__ __forceinline__ const VT* batch_vec(const void* vec, long long stride, int b) {
    return vec ? static_cast<const VT*>(vec) + (size_t)b * (size_t)stride : nullptr;
}

// MODE 0: s = res + gate * x (or x), sum_out = s, y = (norm ? LN(s) : s) * (1 + scale) + shift
// MODE 1: y = res + gate * (LN(x) * (1 + scale) + shift)
// A lane reads every element it owns before it writes one, so sum_out may alias res and y may alias x.
template <class T, class VT, int MODE>
__global__ __launch_bounds__(NORM_WAVES * 64) void adaln_wave_kernel(const AdalnArgs a) {
    constexpr int N = Vec<T>::N;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * NORM_WAVES + (threadIdx.x >> 6);
    if (row >= a.rows) return;
    const int b = row / a.tokens;   // a block of NORM_WAVES rows may span two batch elements: per wave, not per block
    const size_t off = (size_t)row * a.features;
    const T* xr = static_cast<const T*>(a.x) + off;
    const T* rr = a.res ? static_cast<const T*>(a.res) + off : nullptr;
    const VT* gt = static_cast<const VT*>(a.gate_tab);
    const VT* gv = batch_vec<VT>(a.gate_vec, a.gate_stride, b);
    const int nv = a.features / N;  // features % N == 0 guaranteed by the host
    float v[NORM_MAXV][N];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NORM_MAXV; ++i) {
        const int vi = lane + i * 64;
        if (vi < nv) {
            Vec<T> t;
            t.load(xr + vi * N);
            t.to_float(v[i]);
            if (MODE == 0 && rr) {
                Vec<T> r;
                r.load(rr + vi * N);
                float rf[N], g[N];
                r.to_float(rf);
                mod_load<VT, N>(gt, gv, vi * N, 1.f, g);
#pragma unroll
                for (int j = 0; j < N; ++j) v[i][j] = fmaf(g[j], v[i][j], rf[j]);
            }
#pragma unroll
            for (int j = 0; j < N; ++j) sum += v[i][j];
        }
    }
    if (MODE == 0 && a.sum) {
        T* sr = static_cast<T*>(a.sum) + off;
#pragma unroll
        for (int i = 0; i < NORM_MAXV; ++i) {
            const int vi = lane + i * 64;
            if (vi < nv) {
                Vec<T> ov;
                ov.from_float(v[i]);
                ov.store(sr + vi * N);
            }
        }
    }
    if (!a.y) return;
    float mean = 0.f, inv = 1.f;
    if (MODE == 1 || a.norm) {
        mean = wave_sum(sum) / a.features;
        float var = 0.f;
#pragma unroll
        for (int i = 0; i < NORM_MAXV; ++i)
            if (lane + i * 64 < nv) {
#pragma unroll
                for (int j = 0; j < N; ++j) { const float d = v[i][j] - mean; var += d * d; }
            }
        inv = 1.0f / sqrtf(wave_sum(var) / a.features + a.eps);
    }
    const VT* sct = static_cast<const VT*>(a.scale_tab);
    const VT* scv = batch_vec<VT>(a.scale_vec, a.scale_stride, b);
    const VT* sht = static_cast<const VT*>(a.shift_tab);
    const VT* shv = batch_vec<VT>(a.shift_vec, a.shift_stride, b);
    T* yr = static_cast<T*>(a.y) + off;
#pragma unroll
    for (int i = 0; i < NORM_MAXV; ++i) {
        const int vi = lane + i * 64;
        if (vi < nv) {
            float sc[N], sh[N], o[N];
            mod_load<VT, N>(sct, scv, vi * N, 0.f, sc);
            mod_load<VT, N>(sht, shv, vi * N, 0.f, sh);
#pragma unroll
            for (int j = 0; j < N; ++j) o[j] = fmaf((v[i][j] - mean) * inv, 1.0f + sc[j], sh[j]);
            if (MODE == 1) {
                Vec<T> r;
                r.load(rr + vi * N);
                float rf[N], g[N];
                r.to_float(rf);
                mod_load<VT, N>(gt, gv, vi * N, 1.f, g);
#pragma unroll
                for (int j = 0; j < N; ++j) o[j] = fmaf(g[j], o[j], rf[j]);
            }
            Vec<T> ov;
            ov.from_float(o);
            ov.store(yr + vi * N);
        }
    }
}

// Generic fallback: one block per row, scalar accesses, any feature count.  The statistics passes only read; the last pass
// reads an element, then writes it, always in the thread that read it before.
template <class T, class VT, int MODE>
__global__ __launch_bounds__(256) void adaln_block_kernel(const AdalnArgs a) {
    __shared__ float scratch[16];
    const int row = blockIdx.x;
    const int b = row / a.tokens;
    const int features = a.features;
    const size_t off = (size_t)row * features;
    const T* xr = static_cast<const T*>(a.x) + off;
    const T* rr = a.res ? static_cast<const T*>(a.res) + off : nullptr;
    const VT* gt = static_cast<const VT*>(a.gate_tab);
    const VT* gv = batch_vec<VT>(a.gate_vec, a.gate_stride, b);
    auto s_at = [&](int i) {
        float v = to_f(xr[i]);
        if (MODE == 0 && rr) v = fmaf(mod_at<VT>(gt, gv, i, 1.f), v, to_f(rr[i]));
        return v;
    };
    float mean = 0.f, inv = 1.f;
    if (a.y && (MODE == 1 || a.norm)) {
        float sum = 0.f;
        for (int i = threadIdx.x; i < features; i += blockDim.x) sum += s_at(i);
        mean = block_sum(sum, scratch) / features;
        float var = 0.f;
        for (int i = threadIdx.x; i < features; i += blockDim.x) {
            const float d = s_at(i) - mean;
            var += d * d;
        }
        inv = 1.0f / sqrtf(block_sum(var, scratch) / features + a.eps);
    }
    const VT* sct = static_cast<const VT*>(a.scale_tab);
    const VT* scv = batch_vec<VT>(a.scale_vec, a.scale_stride, b);
    const VT* sht = static_cast<const VT*>(a.shift_tab);
    const VT* shv = batch_vec<VT>(a.shift_vec, a.shift_stride, b);
    T* sr = (MODE == 0 && a.sum) ? static_cast<T*>(a.sum) + off : nullptr;
    T* yr = a.y ? static_cast<T*>(a.y) + off : nullptr;
    for (int i = threadIdx.x; i < features; i += blockDim.x) {
        const float s = s_at(i);
        float o = 0.f;
        if (yr) {
            o = fmaf((s - mean) * inv, 1.0f + mod_at<VT>(sct, scv, i, 0.f), mod_at<VT>(sht, shv, i, 0.f));
            if (MODE == 1) o = fmaf(mod_at<VT>(gt, gv, i, 1.f), o, to_f(rr[i]));
        }
        if (sr) sr[i] = from_f<T>(s);
        if (yr) yr[i] = from_f<T>(o);
    }
}

static bool adaln_aligned(const AdalnArgs& a, size_t vec_item) {
    const void* ptrs[] = {a.x, a.res, a.sum, a.y, a.gate_tab, a.gate_vec, a.scale_tab, a.scale_vec, a.shift_tab, a.shift_vec};
    for (const void* p : ptrs)
        if (p && !aligned16(p)) return false;   // absent operands are never read
    const long long strides[] = {a.gate_vec ? a.gate_stride : 0, a.scale_vec ? a.scale_stride : 0, a.shift_vec ? a.shift_stride : 0};
    for (long long s : strides)
        if (((size_t)s * vec_item) % 16) return false;
    return true;
}

template <class T, class VT, int MODE> static pgk_status launch_adaln(const AdalnArgs& a, hipStream_t st) {
    // fp32 vectors under 16-bit rows are read as two 16-byte halves of a row vector, so the row's item size decides
    if (adaln_pick(a.features, sizeof(T), adaln_aligned(a, sizeof(VT))) == NORM_WAVE)      // base_plan.h
        adaln_wave_kernel<T, VT, MODE><<<ceil_div(a.rows, NORM_WAVES), NORM_WAVES * 64, 0, st>>>(a);
    else
        adaln_block_kernel<T, VT, MODE><<<a.rows, 256, 0, st>>>(a);
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

template <class T, class VT> static pgk_status launch_adaln_mode(const AdalnArgs& a, int mode, hipStream_t st) {
    return mode ? launch_adaln<T, VT, 1>(a, st) : launch_adaln<T, VT, 0>(a, st);
}

// ---- patchify / unpatchify: a thread per output element, pure moves ------------------------------------------------------------
template <class U>
__global__ __launch_bounds__(EW_BLOCK) void patchify_kernel(const U* in, U* out, size_t total, int C, int H, int W, int p) {
    const int hp = H / p, wp = W / p, cols = C * p * p;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t o = blockIdx.x * (size_t)blockDim.x + threadIdx.x; o < total; o += stride) {
        const int col = (int)(o % cols);
        const size_t row = o / cols;
        const int pw = col % p, ph = (col / p) % p, c = col / (p * p);
        const int w = (int)(row % wp), h = (int)((row / wp) % hp);
        const size_t b = row / ((size_t)wp * hp);
        out[o] = in[((b * C + c) * H + (size_t)h * p + ph) * W + (size_t)w * p + pw];
    }
}

template <class U>
__global__ __launch_bounds__(EW_BLOCK) void unpatchify_kernel(const U* in, U* out, size_t total, int Co, int H, int W, int p) {
    const int hp = H / p, wp = W / p;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t o = blockIdx.x * (size_t)blockDim.x + threadIdx.x; o < total; o += stride) {
        const int xx = (int)(o % W), yy = (int)((o / W) % H);
        const int c = (int)((o / ((size_t)W * H)) % Co);
        const size_t b = o / ((size_t)W * H * Co);
        const int h = yy / p, ph = yy % p, w = xx / p, pw = xx % p;
        out[o] = in[((b * hp + h) * wp + w) * ((size_t)p * p * Co) + (size_t)(ph * p + pw) * Co + c];
    }
}

static pgk_status check_patch(const char* name, const void* in, const void* out, int B, int C, int H, int W, int p, pgk_dtype dt) {
    PGK_REQUIRE(in && out, "%s: null pointer", name);
    PGK_REQUIRE(B >= 0 && C > 0 && H > 0 && W > 0 && p >= 1, "%s: bad shape B=%d C=%d H=%d W=%d p=%d", name, B, C, H, W, p);
    PGK_REQUIRE(H % p == 0 && W % p == 0, "%s: H=%d and W=%d must be multiples of the patch size %d", name, H, W, p);
    PGK_REQUIRE((long long)C * p * p <= 0x7fffffffLL, "%s: C * p * p = %lld exceeds int32", name, (long long)C * p * p);
    PGK_REQUIRE(dtype_size(dt) == 2 || dtype_size(dt) == 4, "%s: needs a 2- or 4-byte dtype, got %d", name, (int)dt);
    return PGK_OK;
}

}  // namespace pgk

using namespace pgk;

extern "C" {

pgk_status pgk_adaln_fused(const void* x, const void* residual, void* sum_out, void* y, const void* gate_tab, const void* gate_vec,
                           int64_t gate_stride, const void* scale_tab, const void* scale_vec, int64_t scale_stride,
                           const void* shift_tab, const void* shift_vec, int64_t shift_stride, int batch, int tokens, int features,
                           float eps, int norm, int mode, pgk_dtype dt, pgk_dtype vec_dt, pgk_stream s) {
    PGK_REQUIRE(x, "pgk_adaln_fused: null x");
    PGK_REQUIRE(batch >= 0 && tokens >= 0 && features > 0, "pgk_adaln_fused: bad shape [%d,%d,%d]", batch, tokens, features);
    PGK_REQUIRE((long long)batch * tokens <= 0x7fffffffLL, "pgk_adaln_fused: %lld rows exceed int32", (long long)batch * tokens);
    PGK_REQUIRE(mode == 0 || mode == 1, "pgk_adaln_fused: mode must be 0 or 1, got %d", mode);
    PGK_REQUIRE(gate_stride >= 0 && scale_stride >= 0 && shift_stride >= 0, "pgk_adaln_fused: negative vector stride");
    PGK_REQUIRE(is_float_dtype(dt), "pgk_adaln_fused: unsupported dtype %d", (int)dt);
    PGK_REQUIRE(vec_dt == dt || vec_dt == PGK_F32, "pgk_adaln_fused: vectors must be in the row dtype or float32, got %d", (int)vec_dt);
    if (mode == 0) {
        PGK_REQUIRE(sum_out || y, "pgk_adaln_fused: neither sum_out nor y is given");
        PGK_REQUIRE(residual || !(gate_tab || gate_vec), "pgk_adaln_fused: a gate needs a residual");
    } else {
        PGK_REQUIRE(residual && y && !sum_out, "pgk_adaln_fused: mode 1 needs residual and y and writes no sum_out");
    }
    if (!batch || !tokens) return PGK_OK;
    const AdalnArgs a{x, residual, sum_out, y, gate_tab, gate_vec, scale_tab, scale_vec, shift_tab, shift_vec,
                      (long long)gate_stride, (long long)scale_stride, (long long)shift_stride,
                      batch * tokens, tokens, features, norm != 0, eps};
    hipStream_t st = resolve_stream(s);
    if (vec_dt == dt) {
        PGK_DISPATCH_FLOAT(dt, "pgk_adaln_fused", return (launch_adaln_mode<T, T>(a, mode, st)));
    } else {
        PGK_DISPATCH_FLOAT(dt, "pgk_adaln_fused", return (launch_adaln_mode<T, float>(a, mode, st)));
    }
    return PGK_OK;
}

const char* pgk_adaln_plan(int features, pgk_dtype dt, int aligned) {
    if (features <= 0 || !is_float_dtype(dt)) {
        set_error(PGK_ERR_INVALID, "pgk_adaln_plan: bad call features=%d dtype=%d", features, (int)dt);
        return nullptr;
    }
    return adaln_leaf(features, dtype_size(dt), aligned != 0);
}

pgk_status pgk_patchify(const void* in, void* out, int B, int C, int H, int W, int p, pgk_dtype dt, pgk_stream s) {
    if (pgk_status e = check_patch("pgk_patchify", in, out, B, C, H, W, p, dt)) return e;
    const size_t total = (size_t)B * C * H * W;
    if (!total) return PGK_OK;
    hipStream_t st = resolve_stream(s);
    if (dtype_size(dt) == 2)
        patchify_kernel<uint16_t><<<ew_grid(total), EW_BLOCK, 0, st>>>((const uint16_t*)in, (uint16_t*)out, total, C, H, W, p);
    else
        patchify_kernel<uint32_t><<<ew_grid(total), EW_BLOCK, 0, st>>>((const uint32_t*)in, (uint32_t*)out, total, C, H, W, p);
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

pgk_status pgk_unpatchify(const void* in, void* out, int B, int Co, int H, int W, int p, pgk_dtype dt, pgk_stream s) {
    if (pgk_status e = check_patch("pgk_unpatchify", in, out, B, Co, H, W, p, dt)) return e;
    const size_t total = (size_t)B * Co * H * W;
    if (!total) return PGK_OK;
    hipStream_t st = resolve_stream(s);
    if (dtype_size(dt) == 2)
        unpatchify_kernel<uint16_t><<<ew_grid(total), EW_BLOCK, 0, st>>>((const uint16_t*)in, (uint16_t*)out, total, Co, H, W, p);
    else
        unpatchify_kernel<uint32_t><<<ew_grid(total), EW_BLOCK, 0, st>>>((const uint32_t*)in, (uint32_t*)out, total, Co, H, W, p);
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

}  // extern "C"
