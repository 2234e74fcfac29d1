// group_norm / group_norm_silu for gfx950 (reference: native/ops/nn/norm group_norm - and a SiLU computed on the host).
//   y = (x - mean_g) / sqrt(var_g + eps) * gamma[c] + beta[c]  (then v / (1 + exp(-v)) with act), population variance over
// the (C / G) * HW elements of group g of one image; x is [N,C,HW] or channels-last [N,HW,C].  fp32 math, one rounding.
//
// STATISTICS are (count, mean, M2) triples, never sum / sum of squares: a VAE decoder's last stage has groups of 4 channels x
// 1M pixels with a mean far from zero, where E[x^2] - E[x]^2 in fp32 loses every digit of the variance.  A thread takes a
// vector of VW elements, forms its mean and M2 exactly as a two-pass over the registers, and merges the triple into its
// running one with Chan's formula (VW == 1 is Welford's update); lanes merge down the wave (shuffle-down tree), the waves'
// triples are merged in wave order by every thread.  Every order is fixed and there is no atomic: two runs give the same bits.
//
// Plans.  "block": one workgroup per (image, group) computes the statistics and normalises, one launch.  "split", for
// groups too large for one workgroup to stream: launch 1 writes one triple per (image, group, pixel chunk); launch 2, on the
// same grid, re-merges the group's triples in chunk order in every workgroup and normalises its chunk.  Channels-last 16-bit
// groups narrower than a 16-byte vector take the split plan's row form (group_norm_rows_kernel below).
// Global offsets are size_t; a group has fewer than 2^31 elements (checked).

#include <cstdlib>
#include <cstring>

#include "pgk_device.hip.h"
#include "pgk_internal.h"

namespace pgk {

constexpr int GN_THREADS = 256;
constexpr int GN_CHUNK_ELEMS = 8192;        // elements of one group a split-plan workgroup owns
constexpr int GN_SPLIT_ABOVE = 32768;       // group elements above which the split plan is chosen

struct GnArgs {
    const void* x; const void* gamma; const void* beta; void* y;
    float* part;                            // [N][G][nchunks][3]
    int N, C, HW, G, cg, chunk_px, nchunks, act;
    float eps;
};

struct Wf { float n, mean, m2; };

// a <- a merged with b (Chan et al.); an empty b leaves a as it is
__device__ __forceinline__ void wf_merge(Wf& a, const Wf& b) {
    const float n = a.n + b.n;
    if (b.n == 0.f) return;
    const float d = b.mean - a.mean, f = b.n / n;
    a.mean = a.mean + d * f;
    a.m2 = a.m2 + b.m2 + d * d * a.n * f;
    a.n = n;
}

// every thread's triple -> the workgroup's, the same bits in every thread.  lds holds GN_THREADS / 64 triples.
__device__ __forceinline__ Wf wf_block(Wf w, Wf* lds) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        Wf o;
        o.n = __shfl_down(w.n, off, 64);
        o.mean = __shfl_down(w.mean, off, 64);
        o.m2 = __shfl_down(w.m2, off, 64);
        wf_merge(w, o);                      // lane 0 ends with lanes 0..63 merged as a fixed tree
    }
    __syncthreads();                         // lds may still be read from a previous call
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = w;
    __syncthreads();
    Wf r{0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < GN_THREADS / 64; ++i) wf_merge(r, lds[i]);
    return r;
}

template <class T, int VW> struct alignas(sizeof(T) * VW) GnPack { T e[VW]; };

// Vector i of the workgroup's range [p0, p1) of group g of image n: its offset and the channel of its first element.
// Channels-last: vectors run along the group's channels of one pixel; else along the pixels of one channel.
template <bool CL, int VW>
__device__ __forceinline__ void gn_locate(const GnArgs& a, int n, int g, int p0, int inner, int i, size_t& off, int& c) {
    const int q = i / inner, v = i - q * inner;
    if (CL) {
        c = g * a.cg + v * VW;
        off = ((size_t)n * a.HW + p0 + q) * a.C + c;
    } else {
        c = g * a.cg + q;
        off = ((size_t)n * a.C + c) * a.HW + p0 + (size_t)v * VW;
    }
}

// PHASE 0: statistics + normalise (block plan); 1: statistics -> part (split, launch 1); 2: merge part + normalise (launch 2)
template <class T, bool CL, int VW, int PHASE>
__global__ __launch_bounds__(GN_THREADS) void group_norm_kernel(const GnArgs a) {
    __shared__ Wf lds[GN_THREADS / 64];
    const int tid = threadIdx.x, chunk = blockIdx.x, g = blockIdx.y, n = blockIdx.z;
    const int p0 = chunk * a.chunk_px, p1 = min(a.HW, p0 + a.chunk_px), len = p1 - p0;
    const int inner = CL ? a.cg / VW : len / VW;
    const int total = CL ? len * inner : a.cg * inner;
    const T* x = static_cast<const T*>(a.x);
    using Pack = GnPack<T, VW>;
    Wf st{0.f, 0.f, 0.f};
    if (PHASE != 2) {
        for (int i = tid; i < total; i += GN_THREADS) {
            size_t off;
            int c;
            gn_locate<CL, VW>(a, n, g, p0, inner, i, off, c);
            const Pack pk = *reinterpret_cast<const Pack*>(x + off);
            float f[VW], s = 0.f;
#pragma unroll
            for (int j = 0; j < VW; ++j) { f[j] = to_f(pk.e[j]); s += f[j]; }
            Wf b{(float)VW, s * (1.0f / VW), 0.f};
#pragma unroll
            for (int j = 0; j < VW; ++j) { const float d = f[j] - b.mean; b.m2 += d * d; }
            wf_merge(st, b);
        }
        st = wf_block(st, lds);
        if (PHASE == 1) {
            if (tid == 0) {
                float* p = a.part + (((size_t)n * a.G + g) * a.nchunks + chunk) * 3;
                p[0] = st.n; p[1] = st.mean; p[2] = st.m2;
            }
            return;
        }
    } else {
        const float* pg = a.part + ((size_t)n * a.G + g) * a.nchunks * 3;
        for (int k = tid; k < a.nchunks; k += GN_THREADS) wf_merge(st, Wf{pg[k * 3], pg[k * 3 + 1], pg[k * 3 + 2]});
        st = wf_block(st, lds);
    }
    const float mean = st.mean, rstd = 1.0f / sqrtf(st.m2 / st.n + a.eps);
    const T* gamma = static_cast<const T*>(a.gamma);
    const T* beta = static_cast<const T*>(a.beta);
    T* y = static_cast<T*>(a.y);
    for (int i = tid; i < total; i += GN_THREADS) {
        size_t off;
        int c;
        gn_locate<CL, VW>(a, n, g, p0, inner, i, off, c);
        const Pack pk = *reinterpret_cast<const Pack*>(x + off);
        Pack o;
#pragma unroll
        for (int j = 0; j < VW; ++j) {
            const int cj = CL ? c + j : c;
            float v = fmaf((to_f(pk.e[j]) - mean) * rstd, to_f(gamma[cj]), to_f(beta[cj]));
            if (a.act) v = v / (1.0f + expf(-v));
            o.e[j] = from_f<T>(v);
        }
        *reinterpret_cast<Pack*>(y + off) = o;
    }
}

// Split plan for channels-last 16-bit groups NARROWER than a 16-byte vector (1, 2 or 4 channels: a decoder's last stage is 4
// channels x 1M pixels).  The kernel above would read 8 bytes per lane, 2 C bytes apart; here a workgroup owns whole pixel rows of
// a chunk: thread -> (row of the chunk tid / vpr, 16-byte column tid % vpr), consecutive lanes read consecutive 16 bytes, and a
// thread keeps one triple for each of the GPV = 8 / cg groups its column holds.  PHASE 1: per (group, chunk) triple - the threads
// of a column are merged in row order by one thread per group.  PHASE 2: the group's chunks are merged in a fixed order (slice
// t / G takes chunks slice, slice + slices, ...; then the slices in order), then the rows are normalised.
constexpr int GN_ROWS_ELEMS = 32768, GN_ROWS_MAX_CHUNKS = 512;

template <class T, int GPV, int PHASE>
__global__ __launch_bounds__(GN_THREADS) void group_norm_rows_kernel(const GnArgs a) {
    constexpr int CG = 8 / GPV;
    __shared__ Wf lds[GN_THREADS * GPV];
    __shared__ float stat[2 * GN_THREADS];       // mean, 1 / sqrt(var + eps) per group; G <= GN_THREADS
    const int tid = threadIdx.x, chunk = blockIdx.x, n = blockIdx.z;
    const int vpr = a.C / 8, rows = GN_THREADS / vpr, col = tid % vpr, r0 = tid / vpr;
    const int p0 = chunk * a.chunk_px, p1 = min(a.HW, p0 + a.chunk_px);
    const size_t base = (size_t)n * a.HW * a.C + (size_t)col * 8;
    const T* x = static_cast<const T*>(a.x) + base;
    if (PHASE == 1) {
        Wf st[GPV];
#pragma unroll
        for (int g = 0; g < GPV; ++g) st[g] = Wf{0.f, 0.f, 0.f};
        for (int p = p0 + r0; p < p1; p += rows) {
            Vec<T> v;
            v.load(x + (size_t)p * a.C);
            float f[8];
            v.to_float(f);
#pragma unroll
            for (int g = 0; g < GPV; ++g) {
                float s = 0.f;
#pragma unroll
                for (int j = 0; j < CG; ++j) s += f[g * CG + j];
                Wf b{(float)CG, s * (1.0f / CG), 0.f};
#pragma unroll
                for (int j = 0; j < CG; ++j) { const float d = f[g * CG + j] - b.mean; b.m2 += d * d; }
                wf_merge(st[g], b);
            }
        }
#pragma unroll
        for (int g = 0; g < GPV; ++g) lds[tid * GPV + g] = st[g];
        __syncthreads();
        if (tid < a.G) {                          // group tid = column tid / GPV, sub-group tid % GPV
            const int c = tid / GPV, sub = tid % GPV;
            Wf r{0.f, 0.f, 0.f};
            for (int k = 0; k < rows; ++k) wf_merge(r, lds[(k * vpr + c) * GPV + sub]);
            float* pp = a.part + (((size_t)n * a.G + tid) * a.nchunks + chunk) * 3;
            pp[0] = r.n; pp[1] = r.mean; pp[2] = r.m2;
        }
        return;
    }
    const int slices = GN_THREADS / a.G;
    if (tid < slices * a.G) {
        const int g = tid % a.G, slice = tid / a.G;
        const float* pg = a.part + ((size_t)n * a.G + g) * a.nchunks * 3;
        Wf r{0.f, 0.f, 0.f};
        for (int k = slice; k < a.nchunks; k += slices) wf_merge(r, Wf{pg[k * 3], pg[k * 3 + 1], pg[k * 3 + 2]});
        lds[tid] = r;
    }
    __syncthreads();
    if (tid < a.G) {
        Wf r{0.f, 0.f, 0.f};
        for (int k = 0; k < slices; ++k) wf_merge(r, lds[k * a.G + tid]);
        stat[2 * tid] = r.mean;
        stat[2 * tid + 1] = 1.0f / sqrtf(r.m2 / r.n + a.eps);
    }
    __syncthreads();
    float mean[GPV], rstd[GPV], gam[8], bet[8];
#pragma unroll
    for (int g = 0; g < GPV; ++g) { mean[g] = stat[2 * (col * GPV + g)]; rstd[g] = stat[2 * (col * GPV + g) + 1]; }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        gam[j] = to_f(static_cast<const T*>(a.gamma)[col * 8 + j]);
        bet[j] = to_f(static_cast<const T*>(a.beta)[col * 8 + j]);
    }
    T* y = static_cast<T*>(a.y) + base;
    for (int p = p0 + r0; p < p1; p += rows) {
        Vec<T> v;
        v.load(x + (size_t)p * a.C);
        float f[8];
        v.to_float(f);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float o = fmaf((f[j] - mean[j / CG]) * rstd[j / CG], gam[j], bet[j]);
            if (a.act) o = o / (1.0f + expf(-o));
            f[j] = o;
        }
        Vec<T> ov;
        ov.from_float(f);
        ov.store(y + (size_t)p * a.C);
    }
}

static int gn_forced_plan() {
    const char* e = getenv("PGK_GN_SPLIT");
    if (e && strcmp(e, "0") == 0) return 0;
    if (e && strcmp(e, "1") == 0) return 1;
    return -1;
}
static bool gn_shape_ok(int N, int C, int HW, int G) {
    return N > 0 && N <= 65535 && C > 0 && HW > 0 && G > 0 && G <= 65535 && C % G == 0 && (long long)(C / G) * HW < (1LL << 31);
}
static int gn_plan(int C, int HW, int G) {
    const int f = gn_forced_plan();
    if (f >= 0) return f;
    return (long long)(C / G) * HW > GN_SPLIT_ABOVE ? 1 : 0;
}
// pixels per chunk of the split plan: about GN_CHUNK_ELEMS elements of a group, a multiple of 8 so that vectors along the
// pixels never straddle a chunk
static int gn_chunk_px(int cg) {
    int px = GN_CHUNK_ELEMS / cg / 8 * 8;
    return px < 8 ? 8 : px;
}

template <class T, bool CL, int VW>
static pgk_status gn_launch(GnArgs a, int plan, hipStream_t st) {
    if (plan == 0) {
        a.chunk_px = a.HW;
        a.nchunks = 1;
        group_norm_kernel<T, CL, VW, 0><<<dim3(1, a.G, a.N), GN_THREADS, 0, st>>>(a);
        PGK_LAUNCH_CHECK();
        return PGK_OK;
    }
    a.chunk_px = gn_chunk_px(a.cg);
    a.nchunks = ceil_div(a.HW, a.chunk_px);
    void* ws = nullptr;
    if (pgk_status r = pgk_malloc(&ws, (size_t)a.N * a.G * a.nchunks * 3 * sizeof(float))) return r;
    a.part = static_cast<float*>(ws);
    const dim3 grid(a.nchunks, a.G, a.N);
    group_norm_kernel<T, CL, VW, 1><<<grid, GN_THREADS, 0, st>>>(a);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        group_norm_kernel<T, CL, VW, 2><<<grid, GN_THREADS, 0, st>>>(a);
        e = hipGetLastError();
    }
    pgk_free(ws);   // stream-ordered reuse: later work on this stream runs after the kernels above
    PGK_CHECK_HIP(e);
    return PGK_OK;
}

template <class T, int GPV>
static pgk_status gn_rows_launch(GnArgs a, hipStream_t st) {
    int px = GN_ROWS_ELEMS / a.C;
    const int floor_px = ceil_div(a.HW, GN_ROWS_MAX_CHUNKS);
    if (px < floor_px) px = floor_px;
    a.chunk_px = px < 1 ? 1 : px;
    a.nchunks = ceil_div(a.HW, a.chunk_px);
    void* ws = nullptr;
    if (pgk_status r = pgk_malloc(&ws, (size_t)a.N * a.G * a.nchunks * 3 * sizeof(float))) return r;
    a.part = static_cast<float*>(ws);
    const dim3 grid(a.nchunks, 1, a.N);
    group_norm_rows_kernel<T, GPV, 1><<<grid, GN_THREADS, 0, st>>>(a);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        group_norm_rows_kernel<T, GPV, 2><<<grid, GN_THREADS, 0, st>>>(a);
        e = hipGetLastError();
    }
    pgk_free(ws);   // stream-ordered reuse
    PGK_CHECK_HIP(e);
    return PGK_OK;
}

template <class T, bool CL>
static pgk_status gn_dispatch(const GnArgs& a, int plan, hipStream_t st) {
    constexpr int FULL = 16 / (int)sizeof(T);
    // widest vector the layout allows: along the channels of a group (channels-last) or along the pixels of a channel
    const auto fits = [&](int vw) {
        const uintptr_t mask = (uintptr_t)vw * sizeof(T) - 1;
        if (((reinterpret_cast<uintptr_t>(a.x) | reinterpret_cast<uintptr_t>(a.y)) & mask) != 0) return false;
        return CL ? (a.cg % vw == 0 && a.C % vw == 0) : a.HW % vw == 0;
    };
    if constexpr (CL && sizeof(T) == 2) {
        // groups narrower than a vector: whole pixel rows per workgroup (group_norm_rows_kernel)
        const bool rows_ok = plan == 1 && (a.cg == 1 || a.cg == 2 || a.cg == 4) && a.C % 8 == 0 && a.C / 8 <= GN_THREADS &&
                             GN_THREADS % (a.C / 8) == 0 && a.G <= GN_THREADS && aligned16(a.x) && aligned16(a.y);
        if (rows_ok) {
            if (a.cg == 4) return gn_rows_launch<T, 2>(a, st);
            if (a.cg == 2) return gn_rows_launch<T, 4>(a, st);
            return gn_rows_launch<T, 8>(a, st);
        }
    }
    if (fits(FULL)) return gn_launch<T, CL, FULL>(a, plan, st);
    if constexpr (FULL == 8)
        if (fits(4)) return gn_launch<T, CL, 4>(a, plan, st);
    return gn_launch<T, CL, 1>(a, plan, st);
}

}  // namespace pgk

using namespace pgk;

extern "C" {

int pgk_group_norm_plan(int N, int C, int HW, int G, pgk_dtype dt, int channels_last) {
    (void)channels_last;
    if (!gn_shape_ok(N, C, HW, G) || !is_float_dtype(dt)) return -1;
    return gn_plan(C, HW, G);
}

pgk_status pgk_group_norm(const void* x, const void* gamma, const void* beta, void* out, int N, int C, int HW, int G, float eps, int act,
                          int channels_last, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(x && gamma && beta && out, "pgk_group_norm: null pointer");
    PGK_REQUIRE(gn_shape_ok(N, C, HW, G), "pgk_group_norm: bad shape N=%d C=%d HW=%d groups=%d (C %% groups == 0, N and groups <= 65535, "
                                          "a group below 2^31 elements)", N, C, HW, G);
    PGK_REQUIRE(act == 0 || act == 1, "pgk_group_norm: activation %d (0 = none, 1 = silu)", act);
    GnArgs a;
    a.x = x; a.gamma = gamma; a.beta = beta; a.y = out; a.part = nullptr;
    a.N = N; a.C = C; a.HW = HW; a.G = G; a.cg = C / G; a.chunk_px = HW; a.nchunks = 1; a.act = act; a.eps = eps;
    const int plan = gn_plan(C, HW, G);
    hipStream_t st = resolve_stream(s);
    if (channels_last) {
        PGK_DISPATCH_FLOAT(dt, "pgk_group_norm", return (gn_dispatch<T, true>(a, plan, st)));
    } else {
        PGK_DISPATCH_FLOAT(dt, "pgk_group_norm", return (gn_dispatch<T, false>(a, plan, st)));
    }
    return PGK_OK;
}

}  // extern "C"
