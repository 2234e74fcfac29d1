// conv1d for gfx950 (reference: native/ops/conv/conv1d_kernels.cuh - one thread per output element, scalar loop over
// C_in * K).  out[b][m][n] = bias[m] + sum_{c,t} w[m][c][t] * x[b][c][n * stride + t - padding], zeros outside [0, L).
//
// 16-bit dtypes: an implicit GEMM on v_mfma_f32_32x32x16 - M = C_out, N = L_out of one batch element, reduction over
// (tap, C_in), fp32 accumulators, no im2col buffer in global memory.  A workgroup (4 waves, 2 x 2) owns 64 output channels
// x 64 output positions; per chunk of 32 input channels it stages ONE input slab and the chunk's weights of every tap:
//   * slab  [(64 - 1) * stride + K positions][32 channels]: the input has positions contiguous and channels strided, the
//     MFMA wants the reduction index (channels) contiguous per lane, so the transpose happens at STORE time - a thread
//     gathers 8 channels of one position (8 coalesced 2-byte loads) and writes one 16-byte chunk of that position's row.
//     Every tap and every stride then reads the same kind of 16-byte row chunk: output position n at tap t is row
//     n * stride + t.  (The transposing LDS read ds_read_b64_tr_b16 on a [channel][position] slab needs 8-byte aligned
//     lane addresses, which a tap shift of 1-3 positions breaks - silently: DESIGN.md.)
//   * weights [K][64 channels out][32 channels in] from the pre-packed image [K][C_out padded to 64][C_in padded to 32]
//     (conv1d_pack_kernel: weight[C_out][C_in][K] has the tap as its fastest index), 16-byte row-contiguous copies.
//   Rows are 80 bytes apart (64 + 16): 16 consecutive rows start on 16 different 4-bank groups.
//   Tails (C_in % 32, C_out % 64, L_out % 64, the padding region) are ZEROS in LDS - the pack pre-pass pads the weights,
//   the slab store zero-fills - so no lane is masked around an MFMA or an LDS read; only the final store is guarded.
// float32, and any 16-bit call the MFMA kernel declines: a tiled FMA kernel, 64 x 64 outputs per workgroup, 4 x 4 per
// thread, slab of 8 channels reused across (up to 8) taps, fp32 accumulation.
// The epilogue of both: + bias, optional tanh GELU (gelu_tanh, the device function of the gelu op), layout
// [B][C_out][L_out] or channels-last [B][L_out][C_out], optional + add[L_out][C_out] after the activation, one rounding.
// One launch per call, plus the weight pack pre-pass when the caller passes no packed image.

#include <cstdlib>
#include <cstring>

#include "flash_common.hip.h"

namespace pgk {

constexpr int CV_BM = 64, CV_BN = 64, CV_CK = 32, CV_THREADS = 256;
constexpr int CV_PITCH = CV_CK * 2 + 16;          // bytes between LDS rows of the slab and of the weight tile
constexpr size_t CV_LDS_MAX = 64 * 1024;
constexpr int CF_CK = 8, CF_KT = 8, CF_WMAX = 320;  // FMA kernel: channels / taps per stage, slab positions

struct ConvArgs {
    int B, C_in, C_out, L, L_out, K, stride, padding, act, channels_last;
};

// acc + bias -> activation -> (+ add) -> rounded store.  __fadd_rn keeps the add out of an FMA with the GELU's last
// multiply: the fused result is bit for bit what gelu and add give as separate ops on the fp32 values.
template <class T>
__device__ __forceinline__ void conv_store(T* out, const T* add, const ConvArgs& a, int b, int m, int n, float v) {
    if (a.act == 1) v = gelu_tanh(v);
    if (a.channels_last) {
        if (add != nullptr) v = __fadd_rn(v, to_f(add[(size_t)n * a.C_out + m]));
        out[((size_t)b * a.L_out + n) * a.C_out + m] = from_f<T>(v);
    } else {
        out[((size_t)b * a.C_out + m) * a.L_out + n] = from_f<T>(v);
    }
}

// weight [C_out][C_in][K] -> [K][cout_pad][cin_pad], zeros in the padding
__global__ __launch_bounds__(256) void conv1d_pack_kernel(const uint16_t* w, uint16_t* wp, int C_in, int C_out, int K, int cin_pad, int cout_pad) {
    const size_t total = (size_t)K * cout_pad * cin_pad;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % cin_pad), m = (int)((i / cin_pad) % cout_pad), t = (int)(i / ((size_t)cin_pad * cout_pad));
        wp[i] = (m < C_out && c < C_in) ? w[((size_t)m * C_in + c) * K + t] : (uint16_t)0;
    }
}

// win = (CV_BN - 1) * stride + K slab rows; dynamic LDS = (win + K * CV_BM) * CV_PITCH bytes
template <class T>
__global__ __launch_bounds__(CV_THREADS) void conv1d_mfma_kernel(const T* x, const T* wp, const T* bias, const T* add, T* out, ConvArgs a,
                                                                 int cin_pad, int cout_pad, int win) {
    extern __shared__ __attribute__((aligned(16))) char cv_smem[];
    char* xs = cv_smem;                                // [win][CV_PITCH]
    char* wsm = cv_smem + (size_t)win * CV_PITCH;      // [K][CV_BM][CV_PITCH]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, ql = lane & 31, h = lane >> 5;
    const int wm = wid >> 1, wn = wid & 1;
    const int n0 = blockIdx.x * CV_BN, m0 = blockIdx.y * CV_BM, b = blockIdx.z;
    const uint16_t* xb = reinterpret_cast<const uint16_t*>(x) + (size_t)b * a.C_in * a.L;
    const int p0 = n0 * a.stride - a.padding;          // input position of slab row 0
    f32x16_fl acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const char* arow = wsm + (wm * 32 + ql) * CV_PITCH + h * 16;
    const char* brow = xs + (wn * 32 + ql) * a.stride * CV_PITCH + h * 16;

    for (int c0 = 0; c0 < a.C_in; c0 += CV_CK) {
        __syncthreads();     // the previous chunk's fragments are read
        // slab: thread -> (position row w, channel octet o); consecutive lanes take consecutive positions
        for (int i = tid; i < win * (CV_CK / 8); i += CV_THREADS) {
            const int o = i / win, w = i - o * win, p = p0 + w;
            // eight INDEPENDENT loads from clamped (always valid) addresses, zeroed afterwards: guarded loads would each
            // wait for the one before (16 serial memory round trips per chunk)
            const bool pok = p >= 0 && p < a.L;
            const uint16_t* src = xb + (pok ? p : 0);
            uint32_t e[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) e[j] = src[(size_t)min(c0 + o * 8 + j, a.C_in - 1) * a.L];
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (!pok || c0 + o * 8 + j >= a.C_in) e[j] = 0u;
            *reinterpret_cast<uint4*>(xs + w * CV_PITCH + o * 16) =
                make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
        }
        // weights of this chunk, every tap: rows of 32 input channels = four 16-byte chunks, padded image: no guards
        for (int i = tid; i < a.K * CV_BM * (CV_CK / 8); i += CV_THREADS) {
            const int ch = i & 3, row = (i >> 2) & (CV_BM - 1), t = i >> 8;
            const uint4 v = *reinterpret_cast<const uint4*>(wp + ((size_t)t * cout_pad + m0 + row) * cin_pad + c0 + ch * 8);
            *reinterpret_cast<uint4*>(wsm + (t * CV_BM + row) * CV_PITCH + ch * 16) = v;
        }
        __syncthreads();
        for (int t = 0; t < a.K; ++t) {
#pragma unroll
            for (int ks = 0; ks < CV_CK / 16; ++ks) {
                const uint4 af = *reinterpret_cast<const uint4*>(arow + t * (CV_BM * CV_PITCH) + ks * 32);
                const uint4 bf = *reinterpret_cast<const uint4*>(brow + t * CV_PITCH + ks * 32);
                acc = mfma32<T>(af, bf, acc);
            }
        }
    }
    // accumulator layout: column n = lane & 31, rows (r & 3) + 8 (r >> 2) + 4 h
    const int n = n0 + wn * 32 + ql;
    if (n < a.L_out) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (m < a.C_out) conv_store<T>(out, add, a, b, m, n, acc[r] + (bias != nullptr ? to_f(bias[m]) : 0.f));
        }
    }
}

// bn output positions per workgroup (<= 64, chosen by the host so that (bn - 1) * stride + min(K, CF_KT) <= CF_WMAX)
template <class T>
__global__ __launch_bounds__(256) void conv1d_fma_kernel(const T* x, const T* w, const T* bias, const T* add, T* out, ConvArgs a, int bn) {
    __shared__ float xs[CF_CK][CF_WMAX];
    __shared__ __attribute__((aligned(16))) float wl[CF_CK][CF_KT][CV_BM];
    const int tid = threadIdx.x, tn = tid & 15, tm = tid >> 4;      // outputs m0 + 4 tm + i, nb0 + tn + 16 j
    const int nb0 = blockIdx.x * bn, m0 = blockIdx.y * CV_BM, b = blockIdx.z;
    const T* xb = x + (size_t)b * a.C_in * a.L;
    const long long p0 = (long long)nb0 * a.stride - a.padding;
    float acc[4][4];
    int xoff[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        xoff[j] = min(tn + 16 * j, bn - 1) * a.stride;              // positions past bn re-read the last one; never stored
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][j] = 0.f;
    }
    for (int c0 = 0; c0 < a.C_in; c0 += CF_CK) {
        for (int t0 = 0; t0 < a.K; t0 += CF_KT) {
            const int kt = min(CF_KT, a.K - t0), win = (bn - 1) * a.stride + kt;
            __syncthreads();
            for (int i = tid; i < CF_CK * win; i += 256) {
                const int c = i / win, wv = i - c * win, ch = c0 + c;
                const long long p = p0 + t0 + wv;
                const bool ok = ch < a.C_in && p >= 0 && p < a.L;          // load from a clamped address, then select
                const float v = to_f(xb[(size_t)min(ch, a.C_in - 1) * a.L + (ok ? p : 0)]);
                xs[c][wv] = ok ? v : 0.f;
            }
            for (int i = tid; i < CV_BM * CF_CK * kt; i += 256) {
                const int t = i % kt, c = (i / kt) % CF_CK, m = i / (kt * CF_CK), gm = m0 + m, ch = c0 + c;
                const float v = to_f(w[((size_t)min(gm, a.C_out - 1) * a.C_in + min(ch, a.C_in - 1)) * a.K + t0 + t]);
                wl[c][t][m] = (gm < a.C_out && ch < a.C_in) ? v : 0.f;
            }
            __syncthreads();
            for (int c = 0; c < CF_CK; ++c)
                for (int t = 0; t < kt; ++t) {
                    const float4 wv = *reinterpret_cast<const float4*>(&wl[c][t][tm * 4]);
                    const float wf[4] = {wv.x, wv.y, wv.z, wv.w};
                    float xv[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) xv[j] = xs[c][xoff[j] + t];
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(wf[i], xv[j], acc[i][j]);
                }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int nl = tn + 16 * j, n = nb0 + nl;
        if (nl >= bn || n >= a.L_out) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = m0 + tm * 4 + i;
            if (m < a.C_out) conv_store<T>(out, add, a, b, m, n, acc[i][j] + (bias != nullptr ? to_f(bias[m]) : 0.f));
        }
    }
}

static bool conv_mfma_off() {
    const char* e = getenv("PGK_CONV_MFMA");
    return e && strcmp(e, "0") == 0;
}
static inline int conv_cin_pad(int c_in) { return ceil_div(c_in, CV_CK) * CV_CK; }
static inline int conv_cout_pad(int c_out) { return ceil_div(c_out, CV_BM) * CV_BM; }
static inline size_t conv_mfma_lds(int K, int stride) { return ((size_t)(CV_BN - 1) * stride + K + (size_t)K * CV_BM) * CV_PITCH; }
// 1: the MFMA kernel takes the call (16-bit dtype, slab + weight tile fit the LDS, not switched off); 0: the FMA kernel
static int conv_plan(int K, int stride, pgk_dtype dt) {
    return (dt == PGK_BF16 || dt == PGK_F16) && !conv_mfma_off() && conv_mfma_lds(K, stride) <= CV_LDS_MAX ? 1 : 0;
}
static bool conv_shape_ok(int C_in, int C_out, int L, int K, int stride, int padding) {
    return C_in > 0 && C_out > 0 && L > 0 && K > 0 && stride > 0 && padding >= 0 && (long long)L + 2LL * padding < (1LL << 31) &&
           (long long)L + 2LL * padding >= K;
}

template <class T>
static pgk_status conv_mfma_launch(const void* x, const void* w, const void* packed, const void* bias, const void* add, void* out,
                                   const ConvArgs& a, hipStream_t st) {
    const int cin_pad = conv_cin_pad(a.C_in), cout_pad = conv_cout_pad(a.C_out);
    void* ws = nullptr;
    if (packed == nullptr) {
        const size_t elems = (size_t)a.K * cout_pad * cin_pad;
        if (pgk_status r = pgk_malloc(&ws, elems * 2)) return r;
        conv1d_pack_kernel<<<(unsigned)((elems + 255) / 256 > 2048 ? 2048 : (elems + 255) / 256), 256, 0, st>>>(
            (const uint16_t*)w, (uint16_t*)ws, a.C_in, a.C_out, a.K, cin_pad, cout_pad);
        packed = ws;
    }
    const size_t lds = conv_mfma_lds(a.K, a.stride);
    static bool attr_done = false;
    hipError_t e = hipSuccess;
    if (!attr_done) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv1d_mfma_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)CV_LDS_MAX);
        attr_done = e == hipSuccess;
    }
    if (e == hipSuccess) {
        const dim3 grid(ceil_div(a.L_out, CV_BN), ceil_div(a.C_out, CV_BM), a.B);
        conv1d_mfma_kernel<T><<<grid, CV_THREADS, lds, st>>>((const T*)x, (const T*)packed, (const T*)bias, (const T*)add, (T*)out, a, cin_pad,
                                                            cout_pad, (CV_BN - 1) * a.stride + a.K);
        e = hipGetLastError();
    }
    if (ws) pgk_free(ws);   // stream-ordered reuse: later work on this stream runs after the kernels above
    PGK_CHECK_HIP(e);
    return PGK_OK;
}

template <class T>
static pgk_status conv_fma_launch(const void* x, const void* w, const void* bias, const void* add, void* out, const ConvArgs& a, hipStream_t st) {
    const int kt = a.K < CF_KT ? a.K : CF_KT;
    int bn = (CF_WMAX - kt) / a.stride + 1;
    if (bn > CV_BN) bn = CV_BN;
    const long long gx = ceil_div(a.L_out, bn);
    const dim3 grid((unsigned)gx, ceil_div(a.C_out, CV_BM), a.B);
    conv1d_fma_kernel<T><<<grid, 256, 0, st>>>((const T*)x, (const T*)w, (const T*)bias, (const T*)add, (T*)out, a, bn);
    PGK_CHECK_HIP(hipGetLastError());
    return PGK_OK;
}

}  // namespace pgk

using namespace pgk;

extern "C" {

int pgk_conv1d_plan(int C_in, int C_out, int L, int K, int stride, int padding, pgk_dtype dt) {
    if (!conv_shape_ok(C_in, C_out, L, K, stride, padding) || !is_float_dtype(dt)) return -1;
    return conv_plan(K, stride, dt);
}

size_t pgk_conv1d_packed_elems(int C_in, int C_out, int K) {
    if (C_in <= 0 || C_out <= 0 || K <= 0) return 0;
    return (size_t)K * conv_cout_pad(C_out) * conv_cin_pad(C_in);
}

pgk_status pgk_conv1d_pack_weight(const void* weight, void* packed, int C_in, int C_out, int K, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(weight && packed, "pgk_conv1d_pack_weight: null pointer");
    PGK_REQUIRE(C_in > 0 && C_out > 0 && K > 0, "pgk_conv1d_pack_weight: bad shape C_in=%d C_out=%d K=%d", C_in, C_out, K);
    PGK_REQUIRE(dt == PGK_BF16 || dt == PGK_F16, "pgk_conv1d_pack_weight: only the 16-bit kernels read a packed weight (dtype %d)", (int)dt);
    const size_t elems = pgk_conv1d_packed_elems(C_in, C_out, K);
    const size_t blocks = (elems + 255) / 256;
    conv1d_pack_kernel<<<(unsigned)(blocks > 2048 ? 2048 : blocks), 256, 0, resolve_stream(s)>>>((const uint16_t*)weight, (uint16_t*)packed, C_in, C_out,
                                                                                                K, conv_cin_pad(C_in), conv_cout_pad(C_out));
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

pgk_status pgk_conv1d(const void* x, const void* weight, const void* packed_weight, const void* bias, const void* add, void* out, int B,
                      int C_in, int C_out, int L, int K, int stride, int padding, int act, int channels_last, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(x && weight && out, "pgk_conv1d: null pointer");
    PGK_REQUIRE(B > 0 && B <= 65535, "pgk_conv1d: batch %d outside [1, 65535]", B);
    PGK_REQUIRE(conv_shape_ok(C_in, C_out, L, K, stride, padding),
                "pgk_conv1d: bad shape C_in=%d C_out=%d L=%d K=%d stride=%d padding=%d (needs L + 2 * padding >= K)", C_in, C_out, L, K, stride, padding);
    PGK_REQUIRE(ceil_div(C_out, CV_BM) <= 65535, "pgk_conv1d: C_out %d too large", C_out);
    PGK_REQUIRE(act == 0 || act == 1, "pgk_conv1d: activation %d (0 = none, 1 = gelu)", act);
    PGK_REQUIRE(add == nullptr || channels_last, "pgk_conv1d: add needs channels_last");
    const int L_out = (int)(((long long)L + 2LL * padding - K) / stride + 1);
    const ConvArgs a{B, C_in, C_out, L, L_out, K, stride, padding, act, channels_last ? 1 : 0};
    hipStream_t st = resolve_stream(s);
    if (conv_plan(K, stride, dt) && (packed_weight == nullptr || aligned16(packed_weight))) {
        if (dt == PGK_BF16) return conv_mfma_launch<bf16>(x, weight, packed_weight, bias, add, out, a, st);
        return conv_mfma_launch<f16>(x, weight, packed_weight, bias, add, out, a, st);
    }
    PGK_DISPATCH_FLOAT(dt, "pgk_conv1d", return (conv_fma_launch<T>(x, weight, bias, add, out, a, st)));
    return PGK_OK;
}

}  // extern "C"
