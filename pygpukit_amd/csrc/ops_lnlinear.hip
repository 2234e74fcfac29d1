// [build-defined] The linear layer of a LayerNorm transformer's one-token step, in one launch:
//
//   pgk_ln_linear             out[m, n] = act( LN(x[m, :]; gamma, beta, eps) . w[n, :] + bias[n] ) + residual[m, n]      m = 1..8
//   pgk_ln_linear_qkv_cache   the same kernel at m = 1, n = 3 * heads * head_dim, rows scattered to q_out / k_cache / v_cache
//   pgk_embed_token_position  out[:] = tok_table[state[0]][:] + pos_table[state[1]][:]
//
// The weight stream is gemv_core.hip.h's (one wave owns GEMV_R rows at a time, 16 bytes per lane straight to registers,
// fp32 accumulation, row index clamped and the store masked).  What is new is the prologue and the epilogue:
//   * every workgroup stages x[M, K] in LDS AS FP32 and, with a norm, recomputes the row statistics (two-pass mean / population
//     variance, as pgk_layernorm) and overwrites the image with the normalised row - at most K = 5120 values per row, cheaper
//     than a launch.  The normalised activations are never rounded to 16 bits;
//   * issue order: the x (and gamma / beta) loads, THEN the wave's first 16 bytes of each weight row, then the LDS writes,
//     statistics and barriers - the prologue runs under the weight loads' HBM latency (what engine_gemv.hip.h records as
//     measured).  The first chunk of the NEXT row group is requested before the current group's reduction for the same reason.
//     Loads are never guarded per lane: indices are clamped and the results of out-of-range lanes unused;
//   * epilogue in fp32 on lane 0: + bias, gelu_tanh (the gelu op's own function), + residual, ONE rounding at the store.
// No-norm calls whose fp32 image exceeds 64 KB of LDS (large K * M) hold the rows in the dtype, as gemv_kernel does.  Any K, any
// alignment, and norm calls beyond the LDS budget take the generic kernel: one wave per output, scalar loads.
// K is a runtime argument on every path: the dispatcher has no K specialisation.

#include <cstdlib>
#include <type_traits>

#include "gemv_core.hip.h"
#include "pgk_internal.h"

namespace pgk {

constexpr int LNL_BLOCK = 256;             // 4 waves
constexpr int LNL_R = 4;                   // weight rows per wave per trip
constexpr size_t LNL_LDS = 64 * 1024;      // LDS budget of one workgroup

// where a result goes: out[m * N + n], or - k_cache != NULL, m = 1 - row n of the fused q | k | v projection
struct LnScatter {
    void* k_cache;                 // [heads, max_seq, head_dim]
    void* v_cache;
    const int32_t* pos_buf;        // device position, or NULL: h_pos
    int h_pos, heads, head_dim, max_seq;
};

template <class T>
__device__ __forceinline__ void ln_store(float v, int m, int n, int N, const T* bias, const T* residual, T* out, int act,
                                         const LnScatter& sc) {
    if (bias) v += to_f(bias[n]);
    if (act == 1) v = gelu_tanh(v);
    if (residual) v = __fadd_rn(v, to_f(residual[(size_t)m * N + n]));   // never contracted into gelu's last product: the add op's value
    const T o = from_f<T>(v);
    if (!sc.k_cache) {
        out[(size_t)m * N + n] = o;
        return;
    }
    const int d = sc.heads * sc.head_dim;
    if (n < d) {
        out[n] = o;
        return;
    }
    const int pos = min(max(sc.pos_buf ? sc.pos_buf[0] : sc.h_pos, 0), sc.max_seq - 1);   // never outside the cache
    const int j = n < 2 * d ? n - d : n - 2 * d;
    T* cache = reinterpret_cast<T*>(n < 2 * d ? sc.k_cache : sc.v_cache);
    cache[((size_t)(j / sc.head_dim) * sc.max_seq + pos) * sc.head_dim + j % sc.head_dim] = o;
}

// one 16-byte chunk of R weight rows against the M activation rows at k0: gemv_rows' loop body
template <class WT, class XT, int M, int R>
__device__ __forceinline__ void ln_dot_chunk(const uint4 (&raw)[R], const XT* xs, int ldx, int k0, float (&acc)[R][M]) {
    constexpr int NW = WTraits<WT>::NW;
    if constexpr (std::is_same<WT, bf16>::value && std::is_same<XT, bf16>::value) {
        uint4 xr[M];
#pragma unroll
        for (int m = 0; m < M; ++m) xr[m] = *reinterpret_cast<const uint4*>(xs + (size_t)m * ldx + k0);
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int m = 0; m < M; ++m) acc[r][m] = dot8_bf16(raw[r], xr[m], acc[r][m]);
    } else {
        float xf[M][NW];
#pragma unroll
        for (int m = 0; m < M; ++m) XLoad<XT, NW>::load(xs + (size_t)m * ldx + k0, xf[m]);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float wf[NW];
            WTraits<WT>::decode(raw[r], wf);
#pragma unroll
            for (int m = 0; m < M; ++m) {
#pragma unroll
                for (int j = 0; j < NW; ++j) acc[r][m] = fmaf(wf[j], xf[m][j], acc[r][m]);
            }
        }
    }
}

template <class T, class XS>
__device__ __forceinline__ void ln_stage_vec(const Vec<T>& v, XS* dst) {
    if constexpr (std::is_same<XS, T>::value) {
        v.store(dst);
    } else {
        float f[Vec<T>::N];
        v.to_float(f);
#pragma unroll
        for (int i = 0; i < Vec<T>::N / 4; ++i)
            *reinterpret_cast<float4*>(dst + 4 * i) = make_float4(f[4 * i], f[4 * i + 1], f[4 * i + 2], f[4 * i + 3]);
    }
}

// Fast path: K % 8 == 0, x / w (/ gamma / beta) 16-byte aligned, the image within LNL_LDS.  XS = float: fp32 image (required
// with a norm); XS = T: rows held in the dtype (no norm).  LDS: xs[M][K] of XS, then - STAGE_GB - gamma[K], beta[K] of T.
template <class T, class XS, int M>
__global__ __launch_bounds__(LNL_BLOCK) void ln_linear_kernel(const T* x, const T* w, const T* gamma, const T* beta, const T* bias,
                                                              const T* residual, T* out, int K, int N, float eps, int act,
                                                              int stage_gb, LnScatter sc) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NV = Vec<T>::N, NW = WTraits<T>::NW;
    constexpr bool FP32 = std::is_same<XS, float>::value;
    XS* xs = reinterpret_cast<XS*>(smem);
    T* gs = reinterpret_cast<T*>(smem + (size_t)M * K * sizeof(XS));
    T* bs = gs + K;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = blockIdx.x * (LNL_BLOCK / 64) + (tid >> 6);
    const int nwaves = gridDim.x * (LNL_BLOCK / 64);
    const int kvec = K / NV, nvec = M * kvec;
    const bool norm = FP32 && gamma != nullptr;

    // ---- activation loads first (first trip in registers: the whole image when M * K <= 256 vectors) ...
    Vec<T> x0, g0, b0;
    x0.load(x + (size_t)min(tid, nvec - 1) * NV);
    if (norm && stage_gb) {
        g0.load(gamma + (size_t)min(tid, kvec - 1) * NV);
        b0.load(beta + (size_t)min(tid, kvec - 1) * NV);
    }
    // ---- ... then this wave's first chunk of its first row group (row and k clamped: always a valid address)
    const int kpre = lane * NW < K ? lane * NW : 0;
    uint4 raw[LNL_R];
#pragma unroll
    for (int r = 0; r < LNL_R; ++r) raw[r] = load_nt16(w + (size_t)min(wave * LNL_R + r, N - 1) * K + kpre);

    if (tid < nvec) ln_stage_vec<T, XS>(x0, xs + (size_t)tid * NV);
    for (int i = tid + LNL_BLOCK; i < nvec; i += LNL_BLOCK) {
        Vec<T> v;
        v.load(x + (size_t)i * NV);
        ln_stage_vec<T, XS>(v, xs + (size_t)i * NV);
    }
    if (norm && stage_gb) {
        if (tid < kvec) { g0.store(gs + (size_t)tid * NV); b0.store(bs + (size_t)tid * NV); }
        for (int i = tid + LNL_BLOCK; i < kvec; i += LNL_BLOCK) {
            Vec<T> g, b;
            g.load(gamma + (size_t)i * NV);
            b.load(beta + (size_t)i * NV);
            g.store(gs + (size_t)i * NV);
            b.store(bs + (size_t)i * NV);
        }
    }
    __syncthreads();

    if constexpr (FP32) {
        if (norm) {
            // every wave computes every row's statistics from the image (no cross-wave reduction), then the block normalises
            float mean[M], rstd[M];
            const float inv_k = 1.0f / (float)K;
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const float* row = xs + (size_t)m * K;
                float s = 0.f;
                for (int k = lane; k < K; k += 64) s += row[k];
                mean[m] = wave_sum(s) * inv_k;
                float q = 0.f;
                for (int k = lane; k < K; k += 64) { const float c = row[k] - mean[m]; q = fmaf(c, c, q); }
                rstd[m] = rsqrtf(wave_sum(q) * inv_k + eps);
            }
            __syncthreads();                       // all statistics taken before the image changes
            const T* gsrc = stage_gb ? gs : gamma;
            const T* bsrc = stage_gb ? bs : beta;
            for (int k = tid; k < K; k += LNL_BLOCK) {
                const float g = to_f(gsrc[k]), b = to_f(bsrc[k]);
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    float* p = xs + (size_t)m * K + k;
                    *p = fmaf((*p - mean[m]) * rstd[m], g, b);
                }
            }
            __syncthreads();
        }
    }

    for (int g = wave; g * LNL_R < N; g += nwaves) {
        const int n0 = g * LNL_R;
        const T* wrest[LNL_R];
#pragma unroll
        for (int r = 0; r < LNL_R; ++r) wrest[r] = w + (size_t)min(n0 + r, N - 1) * K + 64 * NW;
        float acc[LNL_R][M];
#pragma unroll
        for (int r = 0; r < LNL_R; ++r)
#pragma unroll
            for (int m = 0; m < M; ++m) acc[r][m] = 0.f;
        if (lane * NW < K) ln_dot_chunk<T, XS, M, LNL_R>(raw, xs, K, lane * NW, acc);
        gemv_rows<T, XS, M, LNL_R>(wrest, xs + 64 * NW, K, K - 64 * NW, lane, acc);      // k >= 64 * NW
        // the next group's first chunk goes out before this group's reductions and stores
        const int gn = g + nwaves;
#pragma unroll
        for (int r = 0; r < LNL_R; ++r) raw[r] = load_nt16(w + (size_t)min(gn * LNL_R + r, N - 1) * K + kpre);
#pragma unroll
        for (int r = 0; r < LNL_R; ++r)
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const float v = wave_sum(acc[r][m]);
                if (lane == 0 && n0 + r < N) ln_store<T>(v, m, n0 + r, N, bias, residual, out, act, sc);
            }
    }
}

// Any K, any alignment, any M * K: one wave per output, scalar loads; the row statistics are recomputed when the wave's row
// changes and the normalised value is formed in fp32 on the fly.
template <class T>
__global__ __launch_bounds__(LNL_BLOCK) void ln_linear_generic_kernel(const T* x, const T* w, const T* gamma, const T* beta,
                                                                      const T* bias, const T* residual, T* out, int M, int K, int N,
                                                                      float eps, int act, LnScatter sc) {
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * (LNL_BLOCK / 64) + (threadIdx.x >> 6);
    const int nwaves = gridDim.x * (LNL_BLOCK / 64);
    const float inv_k = 1.0f / (float)K;
    int cur_m = -1;
    float mean = 0.f, rstd = 1.f;
    for (long long o = wave; o < (long long)M * N; o += nwaves) {
        const int m = (int)(o / N), n = (int)(o % N);
        const T* row = x + (size_t)m * K;
        if (gamma && m != cur_m) {
            float s = 0.f;
            for (int k = lane; k < K; k += 64) s += to_f(row[k]);
            mean = wave_sum(s) * inv_k;
            float q = 0.f;
            for (int k = lane; k < K; k += 64) { const float c = to_f(row[k]) - mean; q = fmaf(c, c, q); }
            rstd = rsqrtf(wave_sum(q) * inv_k + eps);
            cur_m = m;
        }
        float acc = 0.f;
        if (gamma) {
            for (int k = lane; k < K; k += 64)
                acc = fmaf(to_f(w[(size_t)n * K + k]), fmaf((to_f(row[k]) - mean) * rstd, to_f(gamma[k]), to_f(beta[k])), acc);
        } else {
            for (int k = lane; k < K; k += 64) acc = fmaf(to_f(w[(size_t)n * K + k]), to_f(row[k]), acc);
        }
        acc = wave_sum(acc);
        if (lane == 0) ln_store<T>(acc, m, n, N, bias, residual, out, act, sc);
    }
}

template <class T>
__global__ __launch_bounds__(256) void embed_token_position_kernel(const T* tok_table, const T* pos_table, T* out, int hidden,
                                                                   int vocab, int max_pos, const int32_t* state) {
    const int t = min(max(state[0], 0), vocab - 1), p = min(max(state[1], 0), max_pos - 1);
    const T* a = tok_table + (size_t)t * hidden;
    const T* b = pos_table + (size_t)p * hidden;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hidden; i += gridDim.x * blockDim.x)
        out[i] = from_f<T>(__fadd_rn(to_f(a[i]), to_f(b[i])));
}

// the grid rule of ops_gemv.hip's gemv_grid: one row group per wave up to 1024 workgroups (4 per CU), grid-stride beyond
static int lnl_grid(long long rows) {
    const int groups = ceil_div(rows, LNL_R * (LNL_BLOCK / 64));
    return groups < 1 ? 1 : (groups > 1024 ? 1024 : groups);
}

enum { LNL_GENERIC = 0, LNL_FP32_IMAGE = 1, LNL_DTYPE_IMAGE = 2 };

static bool lnl_force_generic() {
    const char* e = getenv("PGK_LN_LINEAR_GENERIC");     // read per call: "1" sends every call to the generic kernel
    return e && e[0] == '1';
}

// which kernel a call takes; *stage_gb: gamma / beta copied to LDS beside the image (when they fit)
static int lnl_plan(int m, int k, int n, pgk_dtype dt, bool norm, bool aligned, int* stage_gb) {
    if (stage_gb) *stage_gb = 0;
    if (m < 1 || m > 8 || k < 1 || n < 1 || !is_float_dtype(dt)) return -1;
    if (lnl_force_generic() || k % 8 != 0 || !aligned) return LNL_GENERIC;
    const size_t esz = dtype_size(dt), image32 = (size_t)m * k * 4;
    if (image32 <= LNL_LDS) {
        if (stage_gb && norm) *stage_gb = image32 + 2 * (size_t)k * esz <= LNL_LDS;
        return LNL_FP32_IMAGE;
    }
    if (!norm && (size_t)m * k * esz <= LNL_LDS) return LNL_DTYPE_IMAGE;
    return LNL_GENERIC;
}

template <class T>
static pgk_status lnl_launch(const void* x_, const void* gamma_, const void* beta_, const void* w_, const void* bias_,
                             const void* residual_, void* out_, int m, int k, int n, float eps, int act, const LnScatter& sc,
                             hipStream_t st) {
    const T *x = (const T*)x_, *gamma = (const T*)gamma_, *beta = (const T*)beta_, *w = (const T*)w_, *bias = (const T*)bias_,
            *residual = (const T*)residual_;
    T* out = (T*)out_;
    const bool aligned = aligned16(x) && aligned16(w) && (!gamma || (aligned16(gamma) && aligned16(beta)));
    int stage_gb = 0;
    const pgk_dtype dt = std::is_same<T, float>::value ? PGK_F32 : std::is_same<T, f16>::value ? PGK_F16 : PGK_BF16;
    const int plan = lnl_plan(m, k, n, dt, gamma != nullptr, aligned, &stage_gb);
    if (plan == LNL_GENERIC) {
        ln_linear_generic_kernel<T><<<lnl_grid((long long)m * n), LNL_BLOCK, 0, st>>>(x, w, gamma, beta, bias, residual, out, m, k, n,
                                                                                       eps, act, sc);
    } else if (plan == LNL_FP32_IMAGE) {
        const size_t lds = (size_t)m * k * 4 + (stage_gb ? 2 * (size_t)k * sizeof(T) : 0);
        switch (m) {
#define PGK_LNL_CASE(MM)                                                                                                           \
    case MM: ln_linear_kernel<T, float, MM><<<lnl_grid(n), LNL_BLOCK, lds, st>>>(x, w, gamma, beta, bias, residual, out, k, n, eps, act, \
                                                                                 stage_gb, sc); break;
            PGK_LNL_CASE(1) PGK_LNL_CASE(2) PGK_LNL_CASE(3) PGK_LNL_CASE(4) PGK_LNL_CASE(5) PGK_LNL_CASE(6) PGK_LNL_CASE(7) PGK_LNL_CASE(8)
#undef PGK_LNL_CASE
        }
    } else {
        if constexpr (!std::is_same<T, float>::value) {          // float32: the dtype image IS the fp32 image
            const size_t lds = (size_t)m * k * sizeof(T);
            switch (m) {
#define PGK_LNL_CASE(MM)                                                                                                           \
    case MM: ln_linear_kernel<T, T, MM><<<lnl_grid(n), LNL_BLOCK, lds, st>>>(x, w, nullptr, nullptr, bias, residual, out, k, n, eps, act, \
                                                                             0, sc); break;
                PGK_LNL_CASE(1) PGK_LNL_CASE(2) PGK_LNL_CASE(3) PGK_LNL_CASE(4) PGK_LNL_CASE(5) PGK_LNL_CASE(6) PGK_LNL_CASE(7) PGK_LNL_CASE(8)
#undef PGK_LNL_CASE
            }
        }
    }
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

static bool lnl_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

}  // namespace pgk

using namespace pgk;

extern "C" {

int pgk_ln_linear_plan(int m, int k, int n, pgk_dtype dt, int norm, int aligned) {
    return lnl_plan(m, k, n, dt, norm != 0, aligned != 0, nullptr);
}

pgk_status pgk_ln_linear(const void* x, const void* gamma, const void* beta, const void* w, const void* bias, const void* residual,
                         void* out, int m, int k, int n, float eps, int act, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(x && w && out, "pgk_ln_linear: null pointer");
    PGK_REQUIRE(m >= 1 && m <= 8, "pgk_ln_linear: m=%d outside [1, 8] (more rows belong to pgk_gemm_nt)", m);
    PGK_REQUIRE(k > 0 && n > 0, "pgk_ln_linear: bad shape K=%d N=%d", k, n);
    PGK_REQUIRE(is_float_dtype(dt), "pgk_ln_linear: unsupported dtype %d", (int)dt);
    PGK_REQUIRE((gamma != nullptr) == (beta != nullptr), "pgk_ln_linear: gamma and beta come together (beta without gamma, or gamma without beta)");
    PGK_REQUIRE(act == 0 || act == 1, "pgk_ln_linear: activation %d (0 = none, 1 = gelu)", act);
    const size_t esz = dtype_size(dt);
    PGK_REQUIRE(!lnl_overlap(x, (size_t)m * k * esz, out, (size_t)m * n * esz), "pgk_ln_linear: x may not alias out");
    hipStream_t st = resolve_stream(s);
    const LnScatter sc = {nullptr, nullptr, nullptr, 0, 0, 0, 0};
    PGK_DISPATCH_FLOAT(dt, "pgk_ln_linear", return (lnl_launch<T>(x, gamma, beta, w, bias, residual, out, m, k, n, eps, act, sc, st)));
    return PGK_OK;
}

pgk_status pgk_ln_linear_qkv_cache(const void* x, const void* gamma, const void* beta, const void* w_qkv, const void* bias_qkv,
                                   void* q_out, void* k_cache, void* v_cache, int k, int heads, int head_dim, int max_seq, float eps,
                                   int h_pos, const int32_t* pos_buf, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(x && w_qkv && q_out && k_cache && v_cache, "pgk_ln_linear_qkv_cache: null pointer");
    PGK_REQUIRE(k > 0 && heads > 0 && head_dim > 0 && max_seq > 0 && (long long)3 * heads * head_dim < (1ll << 31),
                "pgk_ln_linear_qkv_cache: bad shape K=%d heads=%d head_dim=%d max_seq=%d", k, heads, head_dim, max_seq);
    PGK_REQUIRE(is_float_dtype(dt), "pgk_ln_linear_qkv_cache: unsupported dtype %d", (int)dt);
    PGK_REQUIRE((gamma != nullptr) == (beta != nullptr), "pgk_ln_linear_qkv_cache: gamma and beta come together");
    PGK_REQUIRE(pos_buf || (h_pos >= 0 && h_pos < max_seq), "pgk_ln_linear_qkv_cache: position %d outside cache of %d rows", h_pos, max_seq);
    const size_t esz = dtype_size(dt);
    const int d = heads * head_dim;
    PGK_REQUIRE(!lnl_overlap(x, (size_t)k * esz, q_out, (size_t)d * esz), "pgk_ln_linear_qkv_cache: x may not alias q_out");
    const size_t cache_bytes = (size_t)heads * max_seq * head_dim * esz;      // other workgroups still read x while rows are stored
    PGK_REQUIRE(!lnl_overlap(x, (size_t)k * esz, k_cache, cache_bytes) && !lnl_overlap(x, (size_t)k * esz, v_cache, cache_bytes),
                "pgk_ln_linear_qkv_cache: x may not alias k_cache or v_cache");
    hipStream_t st = resolve_stream(s);
    const LnScatter sc = {k_cache, v_cache, pos_buf, h_pos, heads, head_dim, max_seq};
    PGK_DISPATCH_FLOAT(dt, "pgk_ln_linear_qkv_cache",
                       return (lnl_launch<T>(x, gamma, beta, w_qkv, bias_qkv, nullptr, q_out, 1, k, 3 * d, eps, 0, sc, st)));
    return PGK_OK;
}

pgk_status pgk_embed_token_position(const void* tok_table, const void* pos_table, void* out, int hidden, int vocab, int max_pos,
                                    const int32_t* state, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(tok_table && pos_table && out && state, "pgk_embed_token_position: null pointer");
    PGK_REQUIRE(hidden > 0 && vocab > 0 && max_pos > 0, "pgk_embed_token_position: bad shape hidden=%d vocab=%d max_pos=%d", hidden, vocab, max_pos);
    hipStream_t st = resolve_stream(s);
    const int grid = ceil_div(hidden, 256) > 64 ? 64 : ceil_div(hidden, 256);
    PGK_DISPATCH_FLOAT(dt, "pgk_embed_token_position",
                       embed_token_position_kernel<T><<<grid, 256, 0, st>>>((const T*)tok_table, (const T*)pos_table, (T*)out, hidden,
                                                                            vocab, max_pos, state));
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

}  // extern "C"
