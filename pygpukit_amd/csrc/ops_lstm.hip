// LSTM forward, one or two directions (reference: native/ops/nn/recurrent/lstm.inl, lstm_kernels.cuh).
//
//   g   = W_ih . x_t + (b_ih + b_hh) + W_hh . h_{t-1}        gate order i, f, g, o (PyTorch)
//   c_t = sigmoid(f) * c_{t-1} + sigmoid(i) * tanh(g_g)       h_t = sigmoid(o) * tanh(c_t)
//
// Three kernels, all stream-ordered, no host synchronisation, no wait other than a workgroup barrier or a kernel boundary:
//   gate projection  G[d][b][s][4H] = x . W_ih[d]^T + (b_ih[d] + b_hh[d]) in fp32, every timestep and both directions in
//                    one launch (16-bit inputs: v_mfma_f32_16x16x32 with fragments loaded straight from global memory;
//                    float32 inputs: fp32 FMAs on LDS tiles, no operand down-converted);
//   stepped          one launch per timestep for every batch row and both directions: a wave owns one hidden unit, streams
//                    its four W_hh rows once with 16-byte loads against h_{t-1} of up to 8 batch rows in registers;
//   resident         H <= 128: one workgroup per (direction, chunk of 4 batch rows) runs all S steps in ONE launch, W_hh in
//                    registers (two threads per gate row), h exchanged through LDS, c in registers.
// In every dtype the gates, h and c are fp32 for the whole sequence; only what is returned is rounded, once.

#include <cstdlib>
#include <type_traits>

#include "pgk_device.hip.h"
#include "pgk_internal.h"

namespace pgk {

typedef __bf16 bf16x8_ls __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8_ls __attribute__((ext_vector_type(8)));
typedef float f32x4_ls __attribute__((ext_vector_type(4)));

template <class T> __device__ __forceinline__ f32x4_ls mfma16_ls(const uint4& a, const uint4& b, f32x4_ls c);
template <> __device__ __forceinline__ f32x4_ls mfma16_ls<bf16>(const uint4& a, const uint4& b, f32x4_ls c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_ls, a), __builtin_bit_cast(bf16x8_ls, b), c, 0, 0, 0);
}
template <> __device__ __forceinline__ f32x4_ls mfma16_ls<f16>(const uint4& a, const uint4& b, f32x4_ls c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_ls, a), __builtin_bit_cast(f16x8_ls, b), c, 0, 0, 0);
}

// One direction's operands as the kernels see them.
struct LstmDir { const void *w_ih, *w_hh, *b_ih, *b_hh, *h0, *c0; };
struct LstmDirs { LstmDir d[2]; };

// sigmoid(x), or tanh(x) as (1 - e) / (1 + e) with e = exp(-2|x|): one v_exp_f32 and one v_rcp_f32 either way, so the
// resident kernel's lanes (one gate each) do not diverge, and both recurrence paths share the arithmetic
__device__ __forceinline__ float lstm_act(float x, bool is_tanh) {
    const float e = __expf(is_tanh ? -2.f * fabsf(x) : -x);
    const float r = (is_tanh ? 1.f - e : 1.f) * __builtin_amdgcn_rcpf(1.f + e);       // v_rcp_f32: 1 ulp
    return is_tanh ? copysignf(r, x) : r;
}

// the time index direction `d` processes at loop step `step`
__device__ __forceinline__ int lstm_time(int step, int S, int d, int reverse) { return (d == 1 || reverse) ? S - 1 - step : step; }

// ---- gate projection, 16-bit inputs ---------------------------------------------------------------------------------------
// workgroup = 4 waves; wave w: rows m0 + 16 w .. + 16 of x against 64 gate columns.  W_ih is the MFMA's A operand and x its B
// operand, so a lane's four accumulators are four CONSECUTIVE gate columns of one row: a 16-byte store.  K % 8 == 0: a
// lane's 8-element fragment is wholly inside or wholly outside K.
constexpr int PJ_BM = 64, PJ_BN = 64;
template <class T>
__global__ __launch_bounds__(256) void lstm_proj16_kernel(const T* x, LstmDirs dirs, float* G, int M, int N, int K) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, d = blockIdx.z;
    const T* w = static_cast<const T*>(dirs.d[d].w_ih);
    const T* bi = static_cast<const T*>(dirs.d[d].b_ih);
    const T* bh = static_cast<const T*>(dirs.d[d].b_hh);
    const int n0 = blockIdx.x * PJ_BN, m0 = blockIdx.y * PJ_BM + wid * 16;
    if (m0 >= M) return;
    const int r = lane & 15, kq = (lane >> 4) * 8;
    const int xm = m0 + r;
    f32x4_ls acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[nt] = f32x4_ls{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += 32) {
        const int k = k0 + kq;
        const bool kin = k < K;
        uint4 xf = make_uint4(0, 0, 0, 0);
        if (kin && xm < M) xf = *reinterpret_cast<const uint4*>(x + (size_t)xm * K + k);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const int wn = n0 + nt * 16 + r;
            uint4 wf = make_uint4(0, 0, 0, 0);
            if (kin && wn < N) wf = *reinterpret_cast<const uint4*>(w + (size_t)wn * K + k);
            acc[nt] = mfma16_ls<T>(wf, xf, acc[nt]);
        }
    }
    if (xm >= M) return;
    float* grow = G + ((size_t)d * M + xm) * N;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int n = n0 + nt * 16 + (lane >> 4) * 4;          // N = 4H, H % 8 == 0: n..n+3 are inside or outside together
        if (n >= N) continue;
        float4 o;
        o.x = acc[nt][0] + (to_f(bi[n]) + to_f(bh[n]));
        o.y = acc[nt][1] + (to_f(bi[n + 1]) + to_f(bh[n + 1]));
        o.z = acc[nt][2] + (to_f(bi[n + 2]) + to_f(bh[n + 2]));
        o.w = acc[nt][3] + (to_f(bi[n + 3]) + to_f(bh[n + 3]));
        *reinterpret_cast<float4*>(grow + n) = o;
    }
}

// ---- gate projection, float32 inputs: any K, any N -----------------------------------------------------------------------
// 64 x 64 output tile, K in slices of 16 through LDS (stored k-major, +1 padding), 4 x 4 outputs per thread, fp32 FMAs.
constexpr int PF_BK = 16;
__global__ __launch_bounds__(256) void lstm_proj32_kernel(const float* x, LstmDirs dirs, float* G, int M, int N, int K) {
    __shared__ float xs[PF_BK][PJ_BM + 1];
    __shared__ float ws[PF_BK][PJ_BN + 1];
    const int d = blockIdx.z, tid = threadIdx.x;
    const float* w = static_cast<const float*>(dirs.d[d].w_ih);
    const float* bi = static_cast<const float*>(dirs.d[d].b_ih);
    const float* bh = static_cast<const float*>(dirs.d[d].b_hh);
    const int n0 = blockIdx.x * PJ_BN, m0 = blockIdx.y * PJ_BM;
    const int tn = (tid & 15) * 4, tm = (tid >> 4) * 4;
    float acc[4][4] = {};
    for (int k0 = 0; k0 < K; k0 += PF_BK) {
        // 64 rows x 16 k per operand = 1024 elements, 4 per thread; consecutive threads walk k (contiguous in memory)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + i * 256, row = e >> 4, kk = e & 15, k = k0 + kk;
            xs[kk][row] = (m0 + row < M && k < K) ? x[(size_t)(m0 + row) * K + k] : 0.f;
            ws[kk][row] = (n0 + row < N && k < K) ? w[(size_t)(n0 + row) * K + k] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < PF_BK; ++kk) {
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { a[i] = xs[kk][tm + i]; b[i] = ws[kk][tn + i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + tm + i;
        if (m >= M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + tn + j;
            if (n < N) G[((size_t)d * M + m) * N + n] = acc[i][j] + (bi[n] + bh[n]);
        }
    }
}

// ---- stepped recurrence ---------------------------------------------------------------------------------------------------
// state workspace (fp32): h ping [ndir][B][H], h pong [ndir][B][H], c [ndir][B][H]
template <class T>
__global__ void lstm_init_kernel(LstmDirs dirs, float* h, float* c, int BH, int ndir) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= BH * ndir) return;
    const int d = i / BH, e = i - d * BH;
    const T* h0 = static_cast<const T*>(dirs.d[d].h0);
    const T* c0 = static_cast<const T*>(dirs.d[d].c0);
    h[i] = h0 ? to_f(h0[e]) : 0.f;
    c[i] = c0 ? to_f(c0[e]) : 0.f;
}

// VN elements of a T row -> float, 16-byte loads when the row starts allow it (vec), guarded scalar loads otherwise
template <class T>
__device__ __forceinline__ void lstm_load_row(const T* p, int k, int H, bool vec, float (&f)[Vec<T>::N]) {
    constexpr int VN = Vec<T>::N;
    if (vec) {
        Vec<T> v;
        v.load(p + k);
        v.to_float(f);
    } else {
#pragma unroll
        for (int i = 0; i < VN; ++i) f[i] = (k + i < H) ? to_f(p[k + i]) : 0.f;
    }
}
template <int VN>
__device__ __forceinline__ void lstm_load_h(const float* p, int k, int H, bool vec, float (&f)[VN]) {
    if (vec) {
#pragma unroll
        for (int q = 0; q < VN / 4; ++q) {
            const float4 v = *reinterpret_cast<const float4*>(p + k + 4 * q);
            f[4 * q] = v.x; f[4 * q + 1] = v.y; f[4 * q + 2] = v.z; f[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < VN; ++i) f[i] = (k + i < H) ? p[k + i] : 0.f;
    }
}

constexpr int ST_WAVES = 4;        // hidden units per workgroup of the stepped kernel, one per wave
constexpr int ST_MB = 8;           // batch rows of h_{t-1} a wave holds in registers

// grid (ceil(H / 4), ndir, ceil(B / MB)).  Each (b, j, d) has exactly one owner: c is updated in place; h_t goes to the
// other half of the ping-pong because other waves of this launch still read h_{t-1}.
template <class T, int MB>
__global__ __launch_bounds__(ST_WAVES * 64) void lstm_step_kernel(const T* whh_f, const T* whh_b, const float* G, const float* h_in,
                                                                  float* h_out, float* c, T* out, T* h_n, T* c_n, int B, int S,
                                                                  int H, int ndir, int step, int reverse, int last) {
    constexpr int VN = Vec<T>::N;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int j = blockIdx.x * ST_WAVES + wid, d = blockIdx.y, b0 = blockIdx.z * MB;
    if (j >= H) return;
    const int nb = min(MB, B - b0);
    const int t = lstm_time(step, S, d, reverse);
    const T* whh = d ? whh_b : whh_f;
    const bool vec = H % VN == 0;

    // the precomputed gates of this lane's batch row, issued ahead of the weight stream
    float gi = 0.f, gf = 0.f, gg = 0.f, go = 0.f, cv = 0.f;
    const size_t sidx = ((size_t)d * B + b0 + lane) * H + j;
    if (lane < nb) {
        const float* gp = G + (((size_t)d * B + b0 + lane) * S + t) * 4 * H + j;
        gi = gp[0]; gf = gp[H]; gg = gp[2 * (size_t)H]; go = gp[3 * (size_t)H];
        cv = c[sidx];
    }

    float acc[4][MB];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int b = 0; b < MB; ++b) acc[g][b] = 0.f;
    const float* hrow = h_in + ((size_t)d * B + b0) * H;
    for (int k = lane * VN; k < H; k += 64 * VN) {
        float hv[MB][VN];
#pragma unroll
        for (int b = 0; b < MB; ++b) {
            if (b < nb) lstm_load_h<VN>(hrow + (size_t)b * H, k, H, vec, hv[b]);
            else {
#pragma unroll
                for (int i = 0; i < VN; ++i) hv[b][i] = 0.f;
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float wv[VN];
            lstm_load_row<T>(whh + ((size_t)g * H + j) * H, k, H, vec, wv);
#pragma unroll
            for (int b = 0; b < MB; ++b)
#pragma unroll
                for (int i = 0; i < VN; ++i) acc[g][b] = fmaf(wv[i], hv[b][i], acc[g][b]);
        }
    }
    // reduce across the wave; lane b keeps batch row b's four sums
    float si = 0.f, sf = 0.f, sg = 0.f, so = 0.f;
#pragma unroll
    for (int b = 0; b < MB; ++b) {
        const float r0 = wave_sum(acc[0][b]), r1 = wave_sum(acc[1][b]), r2 = wave_sum(acc[2][b]), r3 = wave_sum(acc[3][b]);
        if (lane == b) { si = r0; sf = r1; sg = r2; so = r3; }
    }
    if (lane >= nb) return;
    const float ig = lstm_act(gi + si, false), fg = lstm_act(gf + sf, false), cg = lstm_act(gg + sg, true), og = lstm_act(go + so, false);
    const float cn = fg * cv + ig * cg;
    const float hn = og * lstm_act(cn, true);
    c[sidx] = cn;
    h_out[sidx] = hn;
    out[(((size_t)(b0 + lane)) * S + t) * ndir * H + (size_t)d * H + j] = from_f<T>(hn);
    if (last) { h_n[sidx] = from_f<T>(hn); c_n[sidx] = from_f<T>(cn); }
}

// ---- resident recurrence --------------------------------------------------------------------------------------------------
// H <= HMAX (64 or 128).  Workgroup of 8 * HMAX threads: thread = (unit j = tid / 8, gate g = (tid / 2) % 4, half = tid % 2)
// keeps HMAX / 2 weights of row g*H + j (columns half * HMAX/2 ...) in registers as fp32, zero-padded past H.  Per step:
// dot against h_{t-1} read from LDS (a wave reads two distinct addresses per load: broadcast), one cross-lane add joins the
// halves, each lane applies its own gate's activation, the four gates of a unit meet through four DPP moves inside their
// group of 8 lanes, and every lane of the group carries c in a register.  h_t goes to the other LDS half: one barrier a step.
constexpr int DPP_QUAD_LANE0 = 0x00, DPP_QUAD_LANE2 = 0xAA;     // quad_perm [0,0,0,0] / [2,2,2,2]
constexpr int RS_MB = 4;           // batch rows per workgroup
constexpr int RS_HMAX = 128;       // largest H that runs resident (W_hh fp32 = 64 VGPRs per thread of 1024)

template <class T, int HMAX>
__global__ __launch_bounds__(8 * HMAX) void lstm_resident_kernel(LstmDirs dirs, const float* G, T* out, T* h_n, T* c_n, int B, int S,
                                                                 int H, int ndir, int reverse) {
    constexpr int KPT = HMAX / 2;
    __shared__ __attribute__((aligned(16))) float hs[2][RS_MB][HMAX];
    const int tid = threadIdx.x, j = tid >> 3, g = (tid >> 1) & 3, half = tid & 1;
    const int d = blockIdx.y, b0 = blockIdx.x * RS_MB, nb = min(RS_MB, B - b0);
    const T* whh = static_cast<const T*>(dirs.d[d].w_hh);
    const T* h0 = static_cast<const T*>(dirs.d[d].h0);
    const T* c0 = static_cast<const T*>(dirs.d[d].c0);
    const bool unit = j < H;
    const bool writer = unit && g == 0 && half == 0;
    const bool upper = (tid & 4) != 0;                          // second quad of the unit's 8 lanes: gates g, o

    float w[KPT];
    {
        constexpr int VN = Vec<T>::N;
        const T* wrow = whh + ((size_t)g * H + (unit ? j : 0)) * H;
        const int kb = half * KPT;
        const bool vec = H % VN == 0;                            // then a 16-byte piece is wholly inside or outside the row
#pragma unroll
        for (int i = 0; i < KPT; i += VN) {
            float f[VN];
#pragma unroll
            for (int e = 0; e < VN; ++e) f[e] = 0.f;
            if (unit && kb + i < H) lstm_load_row<T>(wrow, kb + i, H, vec, f);
#pragma unroll
            for (int e = 0; e < VN; ++e) w[i + e] = f[e];
        }
    }
    float cst[RS_MB];
#pragma unroll
    for (int b = 0; b < RS_MB; ++b) cst[b] = (unit && b < nb && c0) ? to_f(c0[(size_t)(b0 + b) * H + j]) : 0.f;
    for (int e = tid; e < RS_MB * HMAX; e += 8 * HMAX) {
        const int b = e / HMAX, k = e - b * HMAX;
        hs[0][b][k] = (b < nb && k < H && h0) ? to_f(h0[(size_t)(b0 + b) * H + k]) : 0.f;
        hs[1][b][k] = 0.f;                                      // the padding past H stays zero in both halves
    }
    __syncthreads();

    const size_t gstride = 4 * (size_t)H;
    const float* gbase_p = G + ((size_t)d * B + b0) * S * gstride + (size_t)g * H + (unit ? j : 0);
    float gnext[RS_MB];
    {
        const int t0 = lstm_time(0, S, d, reverse);
#pragma unroll
        for (int b = 0; b < RS_MB; ++b) gnext[b] = (unit && b < nb) ? gbase_p[((size_t)b * S + t0) * gstride] : 0.f;
    }
    float hlast[RS_MB] = {};
    for (int step = 0; step < S; ++step) {
        const int t = lstm_time(step, S, d, reverse), cur = step & 1;
        float gcur[RS_MB];
#pragma unroll
        for (int b = 0; b < RS_MB; ++b) gcur[b] = gnext[b];
        if (step + 1 < S) {                                      // next step's gates travel while this step computes
            const int tn = lstm_time(step + 1, S, d, reverse);
#pragma unroll
            for (int b = 0; b < RS_MB; ++b)
                if (unit && b < nb) gnext[b] = gbase_p[((size_t)b * S + tn) * gstride];
        }
#pragma unroll
        for (int b = 0; b < RS_MB; ++b) {
            if (b >= nb) continue;                               // workgroup-uniform
            const float4* hp = reinterpret_cast<const float4*>(&hs[cur][b][half * KPT]);
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;         // four chains: the dot is latency, not throughput
#pragma unroll
            for (int q = 0; q < KPT / 4; ++q) {
                const float4 hv = hp[q];
                a0 = fmaf(w[4 * q], hv.x, a0); a1 = fmaf(w[4 * q + 1], hv.y, a1);
                a2 = fmaf(w[4 * q + 2], hv.z, a2); a3 = fmaf(w[4 * q + 3], hv.w, a3);
            }
            float a = (a0 + a1) + (a2 + a3);
            a += dpp_f<DPP_XOR1>(a);                              // the other half of the row
            const float act = lstm_act(gcur[b] + a, g == 2);
            // the group's lanes hold i i f f | g g o o: broadcast inside each quad, then swap the quads (lane l <-> 7 - l)
            const float q0 = dpp_f<DPP_QUAD_LANE0>(act), q2 = dpp_f<DPP_QUAD_LANE2>(act);
            const float m0 = dpp_f<DPP_HALF_MIRROR>(q0), m2 = dpp_f<DPP_HALF_MIRROR>(q2);
            const float ig = upper ? m0 : q0, cg = upper ? q0 : m0, fg = upper ? m2 : q2, og = upper ? q2 : m2;
            const float cn = fg * cst[b] + ig * cg;
            const float hn = og * lstm_act(cn, true);
            cst[b] = cn;
            hlast[b] = hn;
            if (writer) {
                hs[cur ^ 1][b][j] = hn;
                out[((size_t)(b0 + b) * S + t) * ndir * H + (size_t)d * H + j] = from_f<T>(hn);
            }
        }
        __syncthreads();
    }
    if (writer) {
#pragma unroll
        for (int b = 0; b < RS_MB; ++b) {
            if (b >= nb) continue;
            const size_t sidx = ((size_t)d * B + b0 + b) * H + j;
            h_n[sidx] = from_f<T>(hlast[b]);
            c_n[sidx] = from_f<T>(cst[b]);
        }
    }
}

static bool lstm_resident_enabled() {
    const char* e = getenv("PGK_LSTM_RESIDENT");           // 0: stepped path for every size (read per call)
    return !(e && atoi(e) == 0);
}

static bool lstm_use_resident(int hidden) { return hidden >= 1 && hidden <= RS_HMAX && lstm_resident_enabled(); }

template <class T>
static pgk_status lstm_run(const T* x, const LstmDirs& dirs, int ndir, T* out, T* h_n, T* c_n, float* G, float* state, int B, int S,
                           int I, int H, int reverse, hipStream_t st) {
    const int M = B * S, N = 4 * H;
    const dim3 pgrid(ceil_div(N, PJ_BN), ceil_div(M, PJ_BM), ndir);
    if constexpr (std::is_same<T, float>::value)
        hipLaunchKernelGGL(lstm_proj32_kernel, pgrid, dim3(256), 0, st, x, dirs, G, M, N, I);
    else
        hipLaunchKernelGGL(lstm_proj16_kernel<T>, pgrid, dim3(256), 0, st, x, dirs, G, M, N, I);
    PGK_LAUNCH_CHECK();

    if (lstm_use_resident(H)) {
        const dim3 grid(ceil_div(B, RS_MB), ndir);
        if (H <= 64)
            hipLaunchKernelGGL((lstm_resident_kernel<T, 64>), grid, dim3(512), 0, st, dirs, G, out, h_n, c_n, B, S, H, ndir, reverse);
        else
            hipLaunchKernelGGL((lstm_resident_kernel<T, 128>), grid, dim3(1024), 0, st, dirs, G, out, h_n, c_n, B, S, H, ndir, reverse);
        PGK_LAUNCH_CHECK();
        return PGK_OK;
    }

    const int BH = B * H;
    float* hbuf[2] = {state, state + (size_t)ndir * BH};
    float* c = state + 2 * (size_t)ndir * BH;
    hipLaunchKernelGGL(lstm_init_kernel<T>, dim3(ceil_div((long long)ndir * BH, 256)), dim3(256), 0, st, dirs, hbuf[0], c, BH, ndir);
    PGK_LAUNCH_CHECK();
    const T* wf = static_cast<const T*>(dirs.d[0].w_hh);
    const T* wb = static_cast<const T*>(dirs.d[ndir - 1].w_hh);
    const int mb = B >= 8 ? 8 : B >= 4 ? 4 : B >= 2 ? 2 : 1;
    const dim3 grid(ceil_div(H, ST_WAVES), ndir, ceil_div(B, mb)), block(ST_WAVES * 64);
    for (int step = 0; step < S; ++step) {
        const float* hin = hbuf[step & 1];
        float* hout = hbuf[(step & 1) ^ 1];
        const int last = step == S - 1;
#define PGK_LSTM_STEP(MB) \
    hipLaunchKernelGGL((lstm_step_kernel<T, MB>), grid, block, 0, st, wf, wb, G, hin, hout, c, out, h_n, c_n, B, S, H, ndir, step, reverse, last)
        switch (mb) {
            case 8: PGK_LSTM_STEP(8); break;
            case 4: PGK_LSTM_STEP(4); break;
            case 2: PGK_LSTM_STEP(2); break;
            default: PGK_LSTM_STEP(1); break;
        }
#undef PGK_LSTM_STEP
        PGK_LAUNCH_CHECK();
    }
    return PGK_OK;
}

}  // namespace pgk

using namespace pgk;

extern "C" {

int pgk_lstm_plan(int batch, int hidden, pgk_dtype dt) {
    (void)batch; (void)dt;      // W_hh lives in registers as fp32 whatever the storage type, and a workgroup takes 4 batch rows
    return lstm_use_resident(hidden) ? 1 : 0;
}

pgk_status pgk_lstm(const void* x, const pgk_lstm_dir* fwd, const pgk_lstm_dir* bwd, void* out, void* h_n, void* c_n, float* ws_gates,
                    float* ws_state, int B, int S, int I, int H, int reverse, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(x && fwd && out && h_n && c_n && ws_gates && ws_state, "pgk_lstm: null argument");
    PGK_REQUIRE(B >= 1 && S >= 1 && I >= 1 && H >= 1, "pgk_lstm: empty dimension (B %d, S %d, I %d, H %d)", B, S, I, H);
    PGK_REQUIRE(is_float_dtype(dt), "pgk_lstm: unsupported dtype %d", (int)dt);
    PGK_REQUIRE(dt == PGK_F32 || (I % 8 == 0 && H % 8 == 0), "pgk_lstm: 16-bit dtypes need I %% 8 == 0 and H %% 8 == 0 (I %d, H %d)", I, H);
    PGK_REQUIRE(!(bwd && reverse), "pgk_lstm: reverse applies to a single direction only");
    PGK_REQUIRE((long long)B * S * 4 * H < (1ll << 31) && (long long)B * S * I < (1ll << 31) && (long long)4 * H * (I > H ? I : H) < (1ll << 31),
                "pgk_lstm: an operand exceeds 2^31 elements");
    const int ndir = bwd ? 2 : 1;
    LstmDirs dirs;
    for (int d = 0; d < 2; ++d) {
        const pgk_lstm_dir* p = (d == 1 && bwd) ? bwd : fwd;
        PGK_REQUIRE(p->w_ih && p->w_hh && p->b_ih && p->b_hh, "pgk_lstm: null weight or bias");
        dirs.d[d] = LstmDir{p->w_ih, p->w_hh, p->b_ih, p->b_hh, p->h0, p->c0};
    }
    PGK_REQUIRE(aligned16(x) && aligned16(dirs.d[0].w_ih) && aligned16(dirs.d[1].w_ih) && aligned16(dirs.d[0].w_hh) &&
                    aligned16(dirs.d[1].w_hh) && aligned16(ws_gates) && aligned16(ws_state),
                "pgk_lstm: x, weights and workspaces must be 16-byte aligned");
    hipStream_t st = resolve_stream(s);
    PGK_DISPATCH_FLOAT(dt, "pgk_lstm",
                       return lstm_run<T>(static_cast<const T*>(x), dirs, ndir, static_cast<T*>(out), static_cast<T*>(h_n),
                                          static_cast<T*>(c_n), ws_gates, ws_state, B, S, I, H, reverse, st));
    return PGK_OK;
}

}  // extern "C"
