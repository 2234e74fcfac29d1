// conv2d for gfx950 (reference: native/ops/conv/conv2d_kernels.cuh - a float32-only direct kernel, one thread per output).
//   out[n][m][oy][ox] = bias[m] + sum_{c,ky,kx} w[m][c][ky][kx] * X[n][c][oy * sh + ky * dh - ph][ox * sw + kx * dw - pw]
// zeros outside X; X is the input, or with upsample == 2 its nearest-neighbour 2x read through (y >> 1, x >> 1) - the
// upsampled tensor never exists.
//
// 16-bit dtypes, KH == KW in {1, 3}, stride in {1, 2}, dilation 1: an implicit GEMM on v_mfma_f32_32x32x16, the 2-D form of
// ops_conv.hip.  M = C_out, N = a TH x 16 patch of output pixels of one image, reduction over (tap, C_in), fp32 accumulators,
// no im2col buffer.  A workgroup (4 waves, 2 x 2) owns 64 output channels x the patch; a wave owns 32 channels x TH / 2 patch
// rows, i.e. TH / 4 accumulator tiles of 2 rows x 16 columns.  Per chunk of 32 input channels it stages
//   * ONE slab [(TH - 1) * s + K][(16 - 1) * s + K][32 channels]: channels contiguous per slab position (the MFMA's reduction
//     index).  From [N,C,H,W] the transpose happens at store time (8 strided 2-byte loads -> one 16-byte LDS write, as
//     conv1d); from channels-last [N,H,W,C] a slab position's 32 channels are four 16-byte loads.  Tap (ky, kx) of output
//     pixel (py, px) is slab position (py * s + ky, px * s + kx): every tap reads the same slab at a shifted row.
//   * the chunk's weights of every tap [K * K][64][32] from the pre-packed image [K * K][C_out pad 64][C_in pad 32].
//   Rows are 80 bytes apart (64 + 16), as in ops_conv.hip.  3x3, stride 1: TH = 8 -> 14.4 KB slab + 46 KB weights,
//   TH = 16 -> 25.9 KB + 46 KB; LDS is 160 KiB per CU.
//   The padding border and every tail (C_in % 32, C_out % 64, ragged patch rows / columns) are ZEROS in LDS: no lane is
//   masked around an MFMA or an LDS read, only the final store is guarded.
// Everything else (float32, other kernel sizes, dilation, PGK_CONV_MFMA=0): a tiled FMA kernel in the style of
// conv1d_fma_kernel, 64 channels x (4 x 16) pixels per workgroup, 4 x 4 per thread, any K / stride / padding / dilation.
// Both: input and output layout, the upsample and the residual `add` are index computations / an epilogue term of the same
// launch; + bias, + add in fp32, one rounding.
// INDEXING: every global offset is a size_t.  A 1024 x 1024 x 128-channel bf16 activation is 256 MB per image and a batch of
// them passes 2^31 elements; no test reaches that size, so the 64-bit arithmetic below is by construction, not by test.

#include <atomic>
#include <cstdlib>
#include <cstring>

#include "flash_common.hip.h"

namespace pgk {

constexpr int C2_BM = 64, C2_TW = 16, C2_CK = 32, C2_THREADS = 256;
constexpr int C2_PITCH = C2_CK * 2 + 16;
constexpr size_t C2_LDS_MAX = 160 * 1024;
constexpr int C2_MAX_DEVICES = 64;
constexpr int F2_CK = 8, F2_KT = 8, F2_TH = 4, F2_TW = 16, F2_WMAX = 80;

struct Conv2dArgs {
    int N, C_in, C_out, H, W;      // stored input
    int He, We;                    // effective input (after the upsample)
    int Ho, Wo, KH, KW, sh, sw, ph, pw, dh, dw;
    int ush;                       // 0, or 1 for upsample == 2
    int cl_in, cl_out;
};

__device__ __forceinline__ size_t c2_out_off(const Conv2dArgs& a, int n, int m, int oy, int ox) {
    return a.cl_out ? (((size_t)n * a.Ho + oy) * a.Wo + ox) * a.C_out + m : (((size_t)n * a.C_out + m) * a.Ho + oy) * a.Wo + ox;
}
// acc + bias (+ add) -> rounded store; __fadd_rn: the result is what the add op gives on the unfused fp32 value
template <class T>
__device__ __forceinline__ void c2_store(T* out, const T* add, const Conv2dArgs& a, int n, int m, int oy, int ox, float v) {
    const size_t off = c2_out_off(a, n, m, oy, ox);
    if (add != nullptr) v = __fadd_rn(v, to_f(add[off]));
    out[off] = from_f<T>(v);
}

// weight [C_out][C_in][KH][KW] -> [KH * KW][cout_pad][cin_pad], zeros in the padding (the tap is the weight's fastest index)
__global__ __launch_bounds__(256) void conv2d_pack_kernel(const uint16_t* w, uint16_t* wp, int C_in, int C_out, int KK, int cin_pad, int cout_pad) {
    const size_t total = (size_t)KK * cout_pad * cin_pad;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % cin_pad), m = (int)((i / cin_pad) % cout_pad), t = (int)(i / ((size_t)cin_pad * cout_pad));
        wp[i] = (m < C_out && c < C_in) ? w[((size_t)m * C_in + c) * KK + t] : (uint16_t)0;
    }
}

struct alignas(8) C2Pack4 { uint16_t e[4]; };

// K = KH = KW, S = stride, TH patch rows.  Dynamic LDS = (SH * SW + K * K * 64) * C2_PITCH bytes.
// vec_in: channels-last input with C_in % 8 == 0 and a 16-byte aligned base; vec_out: channels-last output (and add) with
// C_out % 4 == 0 and 8-byte aligned bases.
template <class T, int K, int S, int TH>
__global__ __launch_bounds__(C2_THREADS) void conv2d_mfma_kernel(const T* x, const T* wp, const T* bias, const T* add, T* out, Conv2dArgs a,
                                                                 int cin_pad, int cout_pad, int tiles_x, int vec_in, int vec_out) {
    constexpr int SH = (TH - 1) * S + K, SW = (C2_TW - 1) * S + K, SHW = SH * SW, KK = K * K, NT = TH / 4;
    extern __shared__ __attribute__((aligned(16))) char c2_smem[];
    char* xs = c2_smem;                                  // [SH][SW][C2_PITCH]
    char* wsm = c2_smem + (size_t)SHW * C2_PITCH;        // [KK][C2_BM][C2_PITCH]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, ql = lane & 31, h = lane >> 5;
    const int wm = wid >> 1, wn = wid & 1;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int oy0 = ty * TH, ox0 = tx * C2_TW, m0 = blockIdx.y * C2_BM, n = blockIdx.z;
    const int y0 = oy0 * S - a.ph, x0 = ox0 * S - a.pw;  // effective-input coordinates of slab position (0, 0)
    const uint16_t* xb = reinterpret_cast<const uint16_t*>(x) + (size_t)n * a.C_in * a.H * a.W;
    const size_t cstride = a.cl_in ? 1 : (size_t)a.H * a.W, pstride = a.cl_in ? (size_t)a.C_in : 1;
    f32x16_fl acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const char* arow = wsm + (wm * 32 + ql) * C2_PITCH + h * 16;
    const char* brow = xs + ((wn * (TH / 2) + (ql >> 4)) * S * SW + (ql & 15) * S) * C2_PITCH + h * 16;   // accumulator tile 0

    for (int c0 = 0; c0 < a.C_in; c0 += C2_CK) {
        __syncthreads();     // the previous chunk's fragments are read
        if (vec_in) {
            // thread -> (slab position, channel octet): a position's 32 channels are 64 contiguous bytes
            for (int i = tid; i < SHW * 4; i += C2_THREADS) {
                const int w = i >> 2, o = i & 3, sy = w / SW, sx = w - sy * SW, yy = y0 + sy, xx = x0 + sx;
                const bool ok = yy >= 0 && yy < a.He && xx >= 0 && xx < a.We && c0 + o * 8 < a.C_in;
                const size_t pix = ok ? (size_t)(yy >> a.ush) * a.W + (xx >> a.ush) : 0;
                uint4 v = *reinterpret_cast<const uint4*>(xb + pix * a.C_in + (ok ? c0 + o * 8 : 0));
                if (!ok) v = make_uint4(0u, 0u, 0u, 0u);
                *reinterpret_cast<uint4*>(xs + w * C2_PITCH + o * 16) = v;
            }
        } else {
            // thread -> (channel octet, slab position); consecutive lanes take consecutive positions.  Eight independent loads
            // from clamped (always valid) addresses, zeroed afterwards (ops_conv.hip)
            for (int i = tid; i < SHW * 4; i += C2_THREADS) {
                const int o = i / SHW, w = i - o * SHW, sy = w / SW, sx = w - sy * SW, yy = y0 + sy, xx = x0 + sx;
                const bool pok = yy >= 0 && yy < a.He && xx >= 0 && xx < a.We;
                const uint16_t* src = xb + (pok ? (size_t)(yy >> a.ush) * a.W + (xx >> a.ush) : 0) * pstride;
                uint32_t e[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) e[j] = src[(size_t)min(c0 + o * 8 + j, a.C_in - 1) * cstride];
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (!pok || c0 + o * 8 + j >= a.C_in) e[j] = 0u;
                *reinterpret_cast<uint4*>(xs + w * C2_PITCH + o * 16) =
                    make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
            }
        }
        // weights of this chunk, every tap: padded image, no guards
        for (int i = tid; i < KK * C2_BM * 4; i += C2_THREADS) {
            const int ch = i & 3, row = (i >> 2) & (C2_BM - 1), t = i >> 8;
            const uint4 v = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(wp) + ((size_t)t * cout_pad + m0 + row) * cin_pad + c0 + ch * 8);
            *reinterpret_cast<uint4*>(wsm + (t * C2_BM + row) * C2_PITCH + ch * 16) = v;
        }
        __syncthreads();
#pragma unroll
        for (int ky = 0; ky < K; ++ky)
#pragma unroll
            for (int kx = 0; kx < K; ++kx)
#pragma unroll
                for (int ks = 0; ks < C2_CK / 16; ++ks) {
                    const uint4 af = *reinterpret_cast<const uint4*>(arow + (ky * K + kx) * (C2_BM * C2_PITCH) + ks * 32);
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const uint4 bf = *reinterpret_cast<const uint4*>(brow + ((t * 2 * S + ky) * SW + kx) * C2_PITCH + ks * 32);
                        acc[t] = mfma32<T>(af, bf, acc[t]);
                    }
                }
    }
    // accumulator layout: column (pixel) = lane & 31, rows (channels) (r & 3) + 8 (r >> 2) + 4 h
    const int ox = ox0 + (ql & 15);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int oy = oy0 + wn * (TH / 2) + t * 2 + (ql >> 4);
        if (oy >= a.Ho || ox >= a.Wo) continue;
        if (vec_out) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int m = m0 + wm * 32 + 8 * q + 4 * h;
                if (m >= a.C_out) continue;          // C_out % 4 == 0: a quad is whole or absent
                const size_t off = c2_out_off(a, n, m, oy, ox);
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = acc[t][4 * q + j] + (bias != nullptr ? to_f(bias[m + j]) : 0.f);
                if (add != nullptr) {
                    const C2Pack4 ad = *reinterpret_cast<const C2Pack4*>(add + off);
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = __fadd_rn(v[j], to_f(__builtin_bit_cast(T, ad.e[j])));
                }
                C2Pack4 o4;
#pragma unroll
                for (int j = 0; j < 4; ++j) o4.e[j] = __builtin_bit_cast(uint16_t, from_f<T>(v[j]));
                *reinterpret_cast<C2Pack4*>(out + off) = o4;
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (m < a.C_out) c2_store<T>(out, add, a, n, m, oy, ox, acc[t][r] + (bias != nullptr ? to_f(bias[m]) : 0.f));
            }
        }
    }
}

// tw output columns per workgroup (<= 16) and kt taps of one kernel row per stage, chosen by the host so that
// (tw - 1) * sw + (kt - 1) * dw + 1 <= F2_WMAX
template <class T>
__global__ __launch_bounds__(256) void conv2d_fma_kernel(const T* x, const T* w, const T* bias, const T* add, T* out, Conv2dArgs a, int tw,
                                                         int kt_max, int tiles_x) {
    __shared__ float xs[F2_CK][F2_TH][F2_WMAX];
    __shared__ __attribute__((aligned(16))) float wl[F2_CK][F2_KT][C2_BM];
    const int tid = threadIdx.x, tn = tid & 15, tm = tid >> 4;      // outputs m0 + 4 tm + i, (oy0 + j, ox0 + tn)
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int oy0 = ty * F2_TH, ox0 = tx * tw, m0 = blockIdx.y * C2_BM, n = blockIdx.z;
    const size_t hw = (size_t)a.H * a.W;
    const T* xb = x + (size_t)n * a.C_in * hw;
    const size_t cstride = a.cl_in ? 1 : hw, pstride = a.cl_in ? (size_t)a.C_in : 1;
    const int xoff = min(tn, tw - 1) * a.sw;                        // columns past tw re-read the last one; never stored
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int c0 = 0; c0 < a.C_in; c0 += F2_CK)
        for (int ky = 0; ky < a.KH; ++ky)
            for (int kx0 = 0; kx0 < a.KW; kx0 += kt_max) {
                const int kt = min(kt_max, a.KW - kx0), win = (tw - 1) * a.sw + (kt - 1) * a.dw + 1;
                __syncthreads();
                for (int i = tid; i < F2_CK * F2_TH * win; i += 256) {
                    const int c = i / (F2_TH * win), rem = i - c * (F2_TH * win), r = rem / win, wv = rem - r * win, ch = c0 + c;
                    const long long yy = (long long)(oy0 + r) * a.sh + (long long)ky * a.dh - a.ph;
                    const long long xx = (long long)ox0 * a.sw + (long long)kx0 * a.dw - a.pw + wv;
                    const bool ok = ch < a.C_in && yy >= 0 && yy < a.He && xx >= 0 && xx < a.We;   // clamped address, then select
                    const size_t pix = ok ? (size_t)(yy >> a.ush) * a.W + (size_t)(xx >> a.ush) : 0;
                    const float v = to_f(xb[pix * pstride + (size_t)min(ch, a.C_in - 1) * cstride]);
                    xs[c][r][wv] = ok ? v : 0.f;
                }
                for (int i = tid; i < C2_BM * F2_CK * kt; i += 256) {
                    const int t = i % kt, c = (i / kt) % F2_CK, m = i / (kt * F2_CK), gm = m0 + m, ch = c0 + c;
                    const float v = to_f(w[(((size_t)min(gm, a.C_out - 1) * a.C_in + min(ch, a.C_in - 1)) * a.KH + ky) * a.KW + kx0 + t]);
                    wl[c][t][m] = (gm < a.C_out && ch < a.C_in) ? v : 0.f;
                }
                __syncthreads();
                for (int c = 0; c < F2_CK; ++c)
                    for (int t = 0; t < kt; ++t) {
                        const float4 wv = *reinterpret_cast<const float4*>(&wl[c][t][tm * 4]);
                        const float wf[4] = {wv.x, wv.y, wv.z, wv.w};
                        float xv[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) xv[j] = xs[c][j][xoff + t * a.dw];
#pragma unroll
                        for (int i = 0; i < 4; ++i)
#pragma unroll
                            for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(wf[i], xv[j], acc[i][j]);
                    }
            }
    const int ox = ox0 + tn;
    if (tn >= tw || ox >= a.Wo) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int oy = oy0 + j;
        if (oy >= a.Ho) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = m0 + tm * 4 + i;
            if (m < a.C_out) c2_store<T>(out, add, a, n, m, oy, ox, acc[i][j] + (bias != nullptr ? to_f(bias[m]) : 0.f));
        }
    }
}

static bool c2_mfma_off() {
    const char* e = getenv("PGK_CONV_MFMA");
    return e && strcmp(e, "0") == 0;
}
static inline int c2_cin_pad(int c_in) { return ceil_div(c_in, C2_CK) * C2_CK; }
static inline int c2_cout_pad(int c_out) { return ceil_div(c_out, C2_BM) * C2_BM; }
static inline size_t c2_mfma_lds(int K, int S, int th) {
    return ((size_t)((th - 1) * S + K) * ((C2_TW - 1) * S + K) + (size_t)K * K * C2_BM) * C2_PITCH;
}
static int c2_plan(int KH, int KW, int sh, int sw, int dh, int dw, pgk_dtype dt) {
    return (dt == PGK_BF16 || dt == PGK_F16) && !c2_mfma_off() && KH == KW && (KH == 1 || KH == 3) && sh == sw && (sh == 1 || sh == 2) &&
                   dh == 1 && dw == 1 && c2_mfma_lds(KH, sh, 8) <= C2_LDS_MAX
               ? 1
               : 0;
}
static bool c2_shape_ok(int C_in, int C_out, int H, int W, int KH, int KW, int sh, int sw, int ph, int pw, int dh, int dw, int up) {
    if (!(C_in > 0 && C_out > 0 && H > 0 && W > 0 && KH > 0 && KW > 0 && sh > 0 && sw > 0 && ph >= 0 && pw >= 0 && dh > 0 && dw > 0 &&
          (up == 1 || up == 2)))
        return false;
    const long long He = (long long)H * up + 2LL * ph, We = (long long)W * up + 2LL * pw;
    const long long eh = (long long)(KH - 1) * dh + 1, ew = (long long)(KW - 1) * dw + 1;
    return He < (1LL << 30) && We < (1LL << 30) && He >= eh && We >= ew;
}
// patch rows of the MFMA kernel: 16 when the image has them and the grid still covers the chip twice (stride 1 only: the
// stride-2 slab of 16 rows is not instantiated).  PGK_CONV2D_ROWS=8/16 forces the height at stride 1 whatever the image
// (tests run the 16-row kernels on small cases with it; tools/vae_bench.py --tile measures both).
static int c2_tile_rows(const Conv2dArgs& a) {
    if (a.sh != 1) return 8;
    if (const char* e = getenv("PGK_CONV2D_ROWS")) {
        if (strcmp(e, "8") == 0) return 8;
        if (strcmp(e, "16") == 0) return 16;
    }
    if (a.Ho <= 8) return 8;
    const long long wgs16 = (long long)ceil_div(a.Ho, 16) * ceil_div(a.Wo, C2_TW) * ceil_div(a.C_out, C2_BM) * a.N;
    return wgs16 >= 2LL * device_cu_count() ? 16 : 8;
}

template <class T, int K, int S, int TH>
static hipError_t c2_mfma_go(const void* x, const void* packed, const void* bias, const void* add, void* out, const Conv2dArgs& a, int vec_in,
                             int vec_out, hipStream_t st) {
    const size_t lds = c2_mfma_lds(K, S, TH);
    // the LDS limit is a property of (kernel, device): one flag per device, set once; a race sets it twice, which is harmless
    static std::atomic<bool> attr_done[C2_MAX_DEVICES];
    int dev = 0;
    if (const hipError_t e = hipGetDevice(&dev)) return e;
    if (dev < 0 || dev >= C2_MAX_DEVICES || !attr_done[dev].load(std::memory_order_acquire)) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv2d_mfma_kernel<T, K, S, TH>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < C2_MAX_DEVICES) attr_done[dev].store(true, std::memory_order_release);
    }
    const long long tiles_x = ceil_div(a.Wo, C2_TW), tiles_y = ceil_div(a.Ho, TH);
    if (tiles_x * tiles_y >= (1LL << 31)) return hipErrorInvalidConfiguration;   // as c2_fma_launch: the x dimension of the grid
    const dim3 grid((unsigned)(tiles_x * tiles_y), ceil_div(a.C_out, C2_BM), a.N);
    conv2d_mfma_kernel<T, K, S, TH><<<grid, C2_THREADS, lds, st>>>((const T*)x, (const T*)packed, (const T*)bias, (const T*)add, (T*)out, a,
                                                                   c2_cin_pad(a.C_in), c2_cout_pad(a.C_out), (int)tiles_x, vec_in, vec_out);
    return hipGetLastError();
}

template <class T>
static pgk_status c2_mfma_launch(const void* x, const void* w, const void* packed, const void* bias, const void* add, void* out,
                                 const Conv2dArgs& a, hipStream_t st) {
    const int cin_pad = c2_cin_pad(a.C_in), cout_pad = c2_cout_pad(a.C_out), KK = a.KH * a.KW;
    void* ws = nullptr;
    if (packed == nullptr) {
        const size_t elems = (size_t)KK * cout_pad * cin_pad;
        if (pgk_status r = pgk_malloc(&ws, elems * 2)) return r;
        conv2d_pack_kernel<<<(unsigned)((elems + 255) / 256 > 2048 ? 2048 : (elems + 255) / 256), 256, 0, st>>>(
            (const uint16_t*)w, (uint16_t*)ws, a.C_in, a.C_out, KK, cin_pad, cout_pad);
        packed = ws;
    }
    const int vec_in = a.cl_in && a.C_in % 8 == 0 && aligned16(x);
    const int vec_out = a.cl_out && a.C_out % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 7u) == 0 &&
                        (add == nullptr || (reinterpret_cast<uintptr_t>(add) & 7u) == 0);
    const int th = c2_tile_rows(a);
    hipError_t e;
    if (a.KH == 1) {
        if (a.sh == 2) e = c2_mfma_go<T, 1, 2, 8>(x, packed, bias, add, out, a, vec_in, vec_out, st);
        else if (th == 16) e = c2_mfma_go<T, 1, 1, 16>(x, packed, bias, add, out, a, vec_in, vec_out, st);
        else e = c2_mfma_go<T, 1, 1, 8>(x, packed, bias, add, out, a, vec_in, vec_out, st);
    } else {
        if (a.sh == 2) e = c2_mfma_go<T, 3, 2, 8>(x, packed, bias, add, out, a, vec_in, vec_out, st);
        else if (th == 16) e = c2_mfma_go<T, 3, 1, 16>(x, packed, bias, add, out, a, vec_in, vec_out, st);
        else e = c2_mfma_go<T, 3, 1, 8>(x, packed, bias, add, out, a, vec_in, vec_out, st);
    }
    if (ws) pgk_free(ws);   // stream-ordered reuse: later work on this stream runs after the kernels above
    PGK_CHECK_HIP(e);
    return PGK_OK;
}

template <class T>
static pgk_status c2_fma_launch(const void* x, const void* w, const void* bias, const void* add, void* out, const Conv2dArgs& a, hipStream_t st) {
    int kt = a.KW < F2_KT ? a.KW : F2_KT;
    while (kt > 1 && (long long)(kt - 1) * a.dw + 1 > F2_WMAX) --kt;
    long long tw = (F2_WMAX - ((long long)(kt - 1) * a.dw + 1)) / a.sw + 1;
    if (tw > F2_TW) tw = F2_TW;
    if (tw < 1) tw = 1;
    const long long tiles_x = ceil_div(a.Wo, tw), tiles_y = ceil_div(a.Ho, F2_TH);
    if (tiles_x * tiles_y >= (1LL << 31)) return set_error(PGK_ERR_INVALID, "pgk_conv2d: %lld x %lld output tiles exceed the grid", tiles_y, tiles_x);
    const dim3 grid((unsigned)(tiles_x * tiles_y), ceil_div(a.C_out, C2_BM), a.N);
    conv2d_fma_kernel<T><<<grid, 256, 0, st>>>((const T*)x, (const T*)w, (const T*)bias, (const T*)add, (T*)out, a, (int)tw, kt, (int)tiles_x);
    PGK_CHECK_HIP(hipGetLastError());
    return PGK_OK;
}

}  // namespace pgk

using namespace pgk;

extern "C" {

int pgk_conv2d_plan(int C_in, int C_out, int H, int W, int KH, int KW, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h,
                    int dil_w, int upsample, pgk_dtype dt) {
    if (!c2_shape_ok(C_in, C_out, H, W, KH, KW, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, upsample) || !is_float_dtype(dt)) return -1;
    return c2_plan(KH, KW, stride_h, stride_w, dil_h, dil_w, dt);
}

size_t pgk_conv2d_packed_elems(int C_in, int C_out, int KH, int KW) {
    if (C_in <= 0 || C_out <= 0 || KH <= 0 || KW <= 0) return 0;
    return (size_t)KH * KW * c2_cout_pad(C_out) * c2_cin_pad(C_in);
}

pgk_status pgk_conv2d_pack_weight(const void* weight, void* packed, int C_in, int C_out, int KH, int KW, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(weight && packed, "pgk_conv2d_pack_weight: null pointer");
    PGK_REQUIRE(C_in > 0 && C_out > 0 && KH > 0 && KW > 0, "pgk_conv2d_pack_weight: bad shape C_in=%d C_out=%d KH=%d KW=%d", C_in, C_out, KH, KW);
    PGK_REQUIRE(dt == PGK_BF16 || dt == PGK_F16, "pgk_conv2d_pack_weight: only the 16-bit kernels read a packed weight (dtype %d)", (int)dt);
    const size_t elems = pgk_conv2d_packed_elems(C_in, C_out, KH, KW);
    const size_t blocks = (elems + 255) / 256;
    conv2d_pack_kernel<<<(unsigned)(blocks > 2048 ? 2048 : blocks), 256, 0, resolve_stream(s)>>>((const uint16_t*)weight, (uint16_t*)packed, C_in, C_out,
                                                                                                KH * KW, c2_cin_pad(C_in), c2_cout_pad(C_out));
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

pgk_status pgk_conv2d(const void* x, const void* weight, const void* packed_weight, const void* bias, const void* add, void* out, int N,
                      int C_in, int C_out, int H, int W, int KH, int KW, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w,
                      int upsample, int channels_last_in, int channels_last_out, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(x && weight && out, "pgk_conv2d: null pointer");
    PGK_REQUIRE(N > 0 && N <= 65535, "pgk_conv2d: batch %d outside [1, 65535]", N);
    PGK_REQUIRE(c2_shape_ok(C_in, C_out, H, W, KH, KW, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, upsample),
                "pgk_conv2d: bad shape C_in=%d C_out=%d H=%d W=%d K=%dx%d stride=%d,%d padding=%d,%d dilation=%d,%d upsample=%d", C_in, C_out, H, W,
                KH, KW, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, upsample);
    PGK_REQUIRE(ceil_div(C_out, C2_BM) <= 65535, "pgk_conv2d: C_out %d too large", C_out);
    Conv2dArgs a;
    a.N = N; a.C_in = C_in; a.C_out = C_out; a.H = H; a.W = W;
    a.He = H * upsample; a.We = W * upsample;
    a.KH = KH; a.KW = KW; a.sh = stride_h; a.sw = stride_w; a.ph = pad_h; a.pw = pad_w; a.dh = dil_h; a.dw = dil_w;
    a.Ho = (int)(((long long)a.He + 2LL * pad_h - ((long long)(KH - 1) * dil_h + 1)) / stride_h + 1);
    a.Wo = (int)(((long long)a.We + 2LL * pad_w - ((long long)(KW - 1) * dil_w + 1)) / stride_w + 1);
    a.ush = upsample == 2 ? 1 : 0;
    a.cl_in = channels_last_in ? 1 : 0;
    a.cl_out = channels_last_out ? 1 : 0;
    hipStream_t st = resolve_stream(s);
    if (c2_plan(KH, KW, stride_h, stride_w, dil_h, dil_w, dt) && (packed_weight == nullptr || aligned16(packed_weight))) {
        if (dt == PGK_BF16) return c2_mfma_launch<bf16>(x, weight, packed_weight, bias, add, out, a, st);
        return c2_mfma_launch<f16>(x, weight, packed_weight, bias, add, out, a, st);
    }
    PGK_DISPATCH_FLOAT(dt, "pgk_conv2d", return (c2_fma_launch<T>(x, weight, bias, add, out, a, st)));
    return PGK_OK;
}

}  // extern "C"
