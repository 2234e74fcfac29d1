// FLUX row kernels (reference: src/pygpukit/diffusion/models/flux/attention.py, ops.py, pipeline.py).
//
// flux_qk_norm_rope: per-head RMSNorm of Q and of K with learned weights, then interleaved-pair RoPE from a general [S, D] fp32
// table, in place, ONE launch for Q and K of a joint [text | image] sequence whose two parts use different norm weights.  The
// reference runs four rmsnorm, three concat_axis1, two apply_rope and three transpose_0213 for the same result.
//   vector path (head_dim 64 / 128, everything on 16 bytes): a head is head_dim / N lanes of one 16-byte vector each (N = 4 fp32,
//     8 16-bit): 8, 16 or 32 lanes.  A rotation pair (2i, 2i+1) lies inside one lane's vector, so only the sum of squares
//     crosses lanes (DPP / one shuffle, no LDS).  A 256-thread block owns 256 / lanes heads; consecutive heads of a row are
//     consecutive in memory, so a wave reads whole contiguous runs.
//   scalar path (any even head_dim <= 256, or anything off 16 bytes): a wave per head, a lane per pair (two at most).
// Everything in fp32, one rounding at the store.  A lane reads all it owns before it writes, so in place is safe.  The tables
// come from the host: no trigonometry here.  Only the Q and K columns are touched.
//
// flux_gelu_pack: gelu of a contiguous [rows, cols] into columns of a wider destination (the single block's [S, 5 D] operand).
// flux_unpack_latents: [B, h w, C 4] with columns (c, ph, pw) -> [B, C, 2h, 2w], a pure move.
// flow_euler_step: sample_f32 += dt * v, the flow-matching Euler update on float32 latents.

#include "base_plan.h"
#include "pgk_device.hip.h"
#include "pgk_internal.h"

namespace pgk {

constexpr int FLUX_MAX_HEAD_DIM = 256;   // scalar path: a lane holds at most two pairs
constexpr int FLUX_BLOCK = 256;

struct FluxNormRopeArgs {
    void* q; void* k;
    const void* wq_a; const void* wk_a; const void* wq_b; const void* wk_b;
    const float* cos; const float* sin;
    long long row_stride, head_stride;
    long long items;          // rows * 2 * heads
    int seq, split, heads, head_dim;
    float eps;
};

// item -> (row, which, head): heads fastest, then Q before K, then rows
struct FluxItem { long long row; int which, head; };
__device__ __forceinline__ FluxItem flux_item(long long item, int heads) {
    FluxItem it;
    it.head = (int)(item % heads);
    const long long rw = item / heads;
    it.which = (int)(rw & 1);
    it.row = rw >> 1;
    return it;
}

// N consecutive values as fp32 from 16-byte aligned memory: one access, or two for fp32 under 16-bit rows (N == 8)
template <class VT, int N> __device__ __forceinline__ void flux_load_f(const VT* p, float (&f)[N]) {
    if constexpr (sizeof(VT) * N == 16) {
        Vec<VT> t;
        t.load(p);
        t.to_float(f);
    } else {
        static_assert(sizeof(VT) == 4 && N == 8, "fp32 values under 16-bit rows");
        const uint4 lo = *reinterpret_cast<const uint4*>(p), hi = *reinterpret_cast<const uint4*>(p + 4);
        f[0] = __uint_as_float(lo.x); f[1] = __uint_as_float(lo.y); f[2] = __uint_as_float(lo.z); f[3] = __uint_as_float(lo.w);
        f[4] = __uint_as_float(hi.x); f[5] = __uint_as_float(hi.y); f[6] = __uint_as_float(hi.z); f[7] = __uint_as_float(hi.w);
    }
}

// the one formula of both paths: n = x * inv * w; out = n * cos + rot * sin with rot[2i] = -n[2i+1], rot[2i+1] = n[2i]
__device__ __forceinline__ void flux_rotate(float x0, float x1, float inv, float w0, float w1, float c0, float c1, float s0, float s1,
                                            float& o0, float& o1) {
    const float n0 = x0 * inv * w0, n1 = x1 * inv * w1;
    o0 = fmaf(-n1, s0, n0 * c0);
    o1 = fmaf(n0, s1, n1 * c1);
}

template <class T, class WT, int D>
__global__ __launch_bounds__(FLUX_BLOCK) void flux_qk_norm_rope_vec_kernel(const FluxNormRopeArgs a) {
    constexpr int N = Vec<T>::N;
    constexpr int LANES = D / N;     // 8, 16 or 32: an aligned group inside a wave
    static_assert(LANES == 8 || LANES == 16 || LANES == 32, "a head is 8, 16 or 32 lanes");
    const long long t = (long long)blockIdx.x * FLUX_BLOCK + threadIdx.x;
    const long long item = t / LANES;
    if (item >= a.items) return;     // whole groups leave together: the group reduction never sees a missing lane
    const int j0 = (int)(t % LANES) * N;
    const FluxItem it = flux_item(item, a.heads);
    const int p = (int)(it.row % a.seq);
    const bool second = p >= a.split;
    const WT* w = static_cast<const WT*>(it.which ? (second ? a.wk_b : a.wk_a) : (second ? a.wq_b : a.wq_a)) + j0;
    T* x = static_cast<T*>(it.which ? a.k : a.q) + it.row * a.row_stride + (long long)it.head * a.head_stride + j0;
    float v[N], wf[N], cf[N], sf[N], o[N];
    Vec<T> in;
    in.load(x);
    in.to_float(v);
    flux_load_f<WT, N>(w, wf);
    flux_load_f<float, N>(a.cos + (size_t)p * D + j0, cf);
    flux_load_f<float, N>(a.sin + (size_t)p * D + j0, sf);
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < N; ++j) ss = fmaf(v[j], v[j], ss);
    const float inv = 1.0f / sqrtf(group_sum<LANES>(ss) / D + a.eps);
#pragma unroll
    for (int j = 0; j < N; j += 2) flux_rotate(v[j], v[j + 1], inv, wf[j], wf[j + 1], cf[j], cf[j + 1], sf[j], sf[j + 1], o[j], o[j + 1]);
    Vec<T> out;
    out.from_float(o);
    out.store(x);
}

template <class T, class WT>
__global__ __launch_bounds__(FLUX_BLOCK) void flux_qk_norm_rope_scalar_kernel(const FluxNormRopeArgs a) {
    const int lane = threadIdx.x & 63;
    const long long item = (long long)blockIdx.x * (FLUX_BLOCK / 64) + (threadIdx.x >> 6);
    if (item >= a.items) return;     // a whole wave
    const FluxItem it = flux_item(item, a.heads);
    const int p = (int)(it.row % a.seq);
    const bool second = p >= a.split;
    const WT* w = static_cast<const WT*>(it.which ? (second ? a.wk_b : a.wk_a) : (second ? a.wq_b : a.wq_a));
    T* x = static_cast<T*>(it.which ? a.k : a.q) + it.row * a.row_stride + (long long)it.head * a.head_stride;
    const float* cs = a.cos + (size_t)p * a.head_dim;
    const float* sn = a.sin + (size_t)p * a.head_dim;
    const int pairs = a.head_dim / 2;                    // <= 128: two per lane at most
    float v[2][2];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int pr = lane + i * 64;
        v[i][0] = v[i][1] = 0.f;
        if (pr < pairs) {
            v[i][0] = to_f(x[2 * pr]);
            v[i][1] = to_f(x[2 * pr + 1]);
            ss = fmaf(v[i][0], v[i][0], ss);
            ss = fmaf(v[i][1], v[i][1], ss);
        }
    }
    const float inv = 1.0f / sqrtf(wave_sum(ss) / a.head_dim + a.eps);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int pr = lane + i * 64;
        if (pr < pairs) {
            const int j = 2 * pr;
            float o0, o1;
            flux_rotate(v[i][0], v[i][1], inv, to_f(w[j]), to_f(w[j + 1]), cs[j], cs[j + 1], sn[j], sn[j + 1], o0, o1);
            x[j] = from_f<T>(o0);
            x[j + 1] = from_f<T>(o1);
        }
    }
}

enum FluxNormRopeKernel { FLUX_NR_VEC = 0, FLUX_NR_SCALAR = 1 };
inline FluxNormRopeKernel flux_nr_pick(int head_dim, bool aligned) {
    return aligned && (head_dim == 64 || head_dim == 128) ? FLUX_NR_VEC : FLUX_NR_SCALAR;
}
inline const char* flux_nr_leaf(int head_dim, bool aligned) {
    return flux_nr_pick(head_dim, aligned) == FLUX_NR_VEC ? "flux_qk_norm_rope_vec" : "flux_qk_norm_rope_scalar";
}

static bool flux_nr_aligned(const FluxNormRopeArgs& a, size_t item) {
    const void* ptrs[] = {a.q, a.k, a.wq_a, a.wk_a, a.wq_b, a.wk_b, a.cos, a.sin};
    for (const void* p : ptrs)
        if (p && !aligned16(p)) return false;
    return ((size_t)a.row_stride * item) % 16 == 0 && ((size_t)a.head_stride * item) % 16 == 0;
}

template <class T, class WT> static pgk_status launch_flux_nr(const FluxNormRopeArgs& a, hipStream_t st) {
    if (flux_nr_pick(a.head_dim, flux_nr_aligned(a, sizeof(T))) == FLUX_NR_VEC) {
        const long long lanes = a.head_dim / Vec<T>::N;
        const long long blocks = (a.items * lanes + FLUX_BLOCK - 1) / FLUX_BLOCK;
        PGK_REQUIRE(blocks <= 0x7fffffffLL, "pgk_flux_qk_norm_rope: %lld blocks exceed the grid", blocks);
        if (a.head_dim == 64)
            flux_qk_norm_rope_vec_kernel<T, WT, 64><<<(int)blocks, FLUX_BLOCK, 0, st>>>(a);
        else
            flux_qk_norm_rope_vec_kernel<T, WT, 128><<<(int)blocks, FLUX_BLOCK, 0, st>>>(a);
    } else {
        const long long blocks = (a.items + FLUX_BLOCK / 64 - 1) / (FLUX_BLOCK / 64);
        PGK_REQUIRE(blocks <= 0x7fffffffLL, "pgk_flux_qk_norm_rope: %lld blocks exceed the grid", blocks);
        flux_qk_norm_rope_scalar_kernel<T, WT><<<(int)blocks, FLUX_BLOCK, 0, st>>>(a);
    }
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

// ---- gelu into a strided destination ---------------------------------------------------------------------------------------------
// The gelu op's value, bit for bit, in every dtype.  With the activation known at compile time hipcc fuses gelu's last product
// with the float16 conversion into v_fma_mixlo_f16 a, b, 0, and (-0.0) + 0 is +0.0 where the op stores -0.0 (every x below
// about -5.2, where 1 + tanh is exactly 0).  The empty asm keeps the fp32 value whole until the conversion.
__device__ __forceinline__ float gelu_value(float x) {
    float g = gelu_tanh(x);
    asm volatile("" : "+v"(g));
    return g;
}

template <class T>
__global__ __launch_bounds__(EW_BLOCK) void flux_gelu_pack_vec_kernel(const T* x, T* out, size_t vectors, int cols, long long out_stride) {
    constexpr int N = Vec<T>::N;
    const int per_row = cols / N;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < vectors; i += stride) {
        const size_t r = i / per_row;
        const int c = (int)(i % per_row) * N;
        Vec<T> t;
        float f[N];
        t.load(x + i * N);
        t.to_float(f);
#pragma unroll
        for (int j = 0; j < N; ++j) f[j] = gelu_value(f[j]);
        t.from_float(f);
        t.store(out + r * (size_t)out_stride + c);
    }
}

template <class T>
__global__ __launch_bounds__(EW_BLOCK) void flux_gelu_pack_scalar_kernel(const T* x, T* out, size_t total, int cols, long long out_stride) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += stride)
        out[(i / cols) * (size_t)out_stride + (i % cols)] = from_f<T>(gelu_value(to_f(x[i])));
}

// ---- unpack: a thread per output element -----------------------------------------------------------------------------------------
template <class U>
__global__ __launch_bounds__(EW_BLOCK) void flux_unpack_kernel(const U* in, U* out, size_t total, int C, int h, int w) {
    const int H = 2 * h, W = 2 * w;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t o = blockIdx.x * (size_t)blockDim.x + threadIdx.x; o < total; o += stride) {
        const int xx = (int)(o % W), yy = (int)((o / W) % H);
        const int c = (int)((o / ((size_t)W * H)) % C);
        const size_t b = o / ((size_t)W * H * C);
        out[o] = in[((b * h + yy / 2) * w + xx / 2) * ((size_t)C * 4) + (size_t)c * 4 + (yy % 2) * 2 + (xx % 2)];
    }
}

template <class T>
__global__ __launch_bounds__(EW_BLOCK) void flow_euler_kernel(float* sample, const T* v, size_t n, float dt) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += stride) sample[i] = fmaf(dt, to_f(v[i]), sample[i]);
}

}  // namespace pgk

using namespace pgk;

extern "C" {

pgk_status pgk_flux_qk_norm_rope(void* q, void* k, int64_t row_stride, int64_t head_stride, const void* wq_a, const void* wk_a,
                                 const void* wq_b, const void* wk_b, const float* cos, const float* sin, int batch, int seq, int split,
                                 int heads, int head_dim, float eps, pgk_dtype dt, pgk_dtype w_dt, pgk_stream s) {
    PGK_REQUIRE(q && k && cos && sin, "pgk_flux_qk_norm_rope: null pointer");
    PGK_REQUIRE(batch >= 0 && seq >= 0 && heads > 0, "pgk_flux_qk_norm_rope: bad shape batch=%d seq=%d heads=%d", batch, seq, heads);
    PGK_REQUIRE(head_dim > 0 && head_dim % 2 == 0, "pgk_flux_qk_norm_rope: head_dim %d must be even (rotation pairs)", head_dim);
    PGK_REQUIRE(head_dim <= FLUX_MAX_HEAD_DIM, "pgk_flux_qk_norm_rope: head_dim %d exceeds %d", head_dim, FLUX_MAX_HEAD_DIM);
    PGK_REQUIRE(split >= 0 && split <= seq, "pgk_flux_qk_norm_rope: split %d outside [0, %d]", split, seq);
    PGK_REQUIRE(row_stride >= 0 && head_stride >= 0, "pgk_flux_qk_norm_rope: negative stride");
    PGK_REQUIRE(split == 0 || (wq_a && wk_a), "pgk_flux_qk_norm_rope: rows below split %d need wq_a and wk_a", split);
    PGK_REQUIRE(split == seq || (wq_b && wk_b), "pgk_flux_qk_norm_rope: rows from split %d on need wq_b and wk_b", split);
    PGK_REQUIRE(is_float_dtype(dt), "pgk_flux_qk_norm_rope: unsupported dtype %d", (int)dt);
    PGK_REQUIRE(w_dt == dt || w_dt == PGK_F32, "pgk_flux_qk_norm_rope: weights must be in the row dtype or float32, got %d", (int)w_dt);
    if (!batch || !seq) return PGK_OK;
    const FluxNormRopeArgs a{q, k, wq_a, wk_a, wq_b, wk_b, cos, sin, (long long)row_stride, (long long)head_stride,
                             (long long)batch * seq * 2 * heads, seq, split, heads, head_dim, eps};
    hipStream_t st = resolve_stream(s);
    if (w_dt == dt) {
        PGK_DISPATCH_FLOAT(dt, "pgk_flux_qk_norm_rope", return (launch_flux_nr<T, T>(a, st)));
    } else {
        PGK_DISPATCH_FLOAT(dt, "pgk_flux_qk_norm_rope", return (launch_flux_nr<T, float>(a, st)));
    }
    return PGK_OK;
}

const char* pgk_flux_qk_norm_rope_plan(int head_dim, pgk_dtype dt, int aligned) {
    if (head_dim <= 0 || head_dim % 2 || head_dim > FLUX_MAX_HEAD_DIM || !is_float_dtype(dt)) {
        set_error(PGK_ERR_INVALID, "pgk_flux_qk_norm_rope_plan: head_dim %d must be even and within %d, dtype %d a float type", head_dim,
                  FLUX_MAX_HEAD_DIM, (int)dt);
        return nullptr;
    }
    return flux_nr_leaf(head_dim, aligned != 0);
}

pgk_status pgk_flux_gelu_pack(const void* x, void* out, int64_t rows, int cols, int64_t out_stride, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(x && out, "pgk_flux_gelu_pack: null pointer");
    PGK_REQUIRE(rows >= 0 && cols > 0 && out_stride >= cols, "pgk_flux_gelu_pack: bad shape rows=%lld cols=%d out_stride=%lld",
                (long long)rows, cols, (long long)out_stride);
    PGK_REQUIRE(is_float_dtype(dt), "pgk_flux_gelu_pack: unsupported dtype %d", (int)dt);
    if (!rows) return PGK_OK;
    const size_t total = (size_t)rows * cols, item = dtype_size(dt);
    const int n = vec_elems(item);
    const bool vec = aligned16(x) && aligned16(out) && cols % n == 0 && out_stride % n == 0;
    hipStream_t st = resolve_stream(s);
    if (vec) {
        PGK_DISPATCH_FLOAT(dt, "pgk_flux_gelu_pack", (flux_gelu_pack_vec_kernel<T><<<ew_grid(total / n), EW_BLOCK, 0, st>>>(
                                                         (const T*)x, (T*)out, total / n, cols, (long long)out_stride)));
    } else {
        PGK_DISPATCH_FLOAT(dt, "pgk_flux_gelu_pack", (flux_gelu_pack_scalar_kernel<T><<<ew_grid(total), EW_BLOCK, 0, st>>>(
                                                         (const T*)x, (T*)out, total, cols, (long long)out_stride)));
    }
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

pgk_status pgk_flux_unpack_latents(const void* in, void* out, int B, int C, int h, int w, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(in && out, "pgk_flux_unpack_latents: null pointer");
    PGK_REQUIRE(B >= 0 && C > 0 && h > 0 && w > 0, "pgk_flux_unpack_latents: bad shape B=%d C=%d h=%d w=%d", B, C, h, w);
    PGK_REQUIRE((long long)C * 4 <= 0x7fffffffLL && 2LL * h <= 0x7fffffffLL && 2LL * w <= 0x7fffffffLL,
                "pgk_flux_unpack_latents: shape exceeds int32");
    PGK_REQUIRE(dtype_size(dt) == 2 || dtype_size(dt) == 4, "pgk_flux_unpack_latents: needs a 2- or 4-byte dtype, got %d", (int)dt);
    const size_t total = (size_t)B * C * 4 * h * w;
    if (!total) return PGK_OK;
    hipStream_t st = resolve_stream(s);
    if (dtype_size(dt) == 2)
        flux_unpack_kernel<uint16_t><<<ew_grid(total), EW_BLOCK, 0, st>>>((const uint16_t*)in, (uint16_t*)out, total, C, h, w);
    else
        flux_unpack_kernel<uint32_t><<<ew_grid(total), EW_BLOCK, 0, st>>>((const uint32_t*)in, (uint32_t*)out, total, C, h, w);
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

pgk_status pgk_flow_euler_step(float* sample, const void* v, size_t n, float dt_step, pgk_dtype v_dt, pgk_stream s) {
    PGK_REQUIRE(sample && v, "pgk_flow_euler_step: null pointer");
    PGK_REQUIRE(is_float_dtype(v_dt), "pgk_flow_euler_step: unsupported dtype %d", (int)v_dt);
    if (!n) return PGK_OK;
    hipStream_t st = resolve_stream(s);
    PGK_DISPATCH_FLOAT(v_dt, "pgk_flow_euler_step", (flow_euler_kernel<T><<<ew_grid(n), EW_BLOCK, 0, st>>>(sample, (const T*)v, n, dt_step)));
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

}  // extern "C"
