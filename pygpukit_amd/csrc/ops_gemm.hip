// MFMA GEMMs for gfx950 (prefill / batched projections):
//   pgk_gemm_nt : C[M,N] = A[M,K] . W[N,K]^T (+bias)   - the Linear layer on the PyTorch-layout weight
//   pgk_gemm_nn : C[M,N] = A[M,K] . B[K,N]             - the generic ops.matmul
//   pgk_w8a16_gemm_kn : bf16 A, fp8-e4m3 B[K,N] with 128x128 block scales (reference K4 layout)
//   (internal) nt with fp8 W[N,K] + block scales, used by the engine's fp8 prefill
//
// Structure (v1): BM x BN x 64 block tile, 256 threads = 2x2 waves, register-staged into two swizzled LDS
// buffers - the tile types and the loop are gemm_tile_core.hip.h (shared with the grouped expert GEMM);
// this file has the kernel's operand modes, its epilogues and the dispatchers.
// The reference reaches for CUTLASS / cuBLASLt here (native/ops/matmul/matmul.cu:43-354); neither
// exists on this target and nothing is linked in their place.

#include "gemm_epilogues.hip.h"
#include "gemm_plan.h"
#include "gemm_tile_core.hip.h"
#include "pgk_internal.h"

#include <string>

namespace pgk {

template <class T> pgk_status launch_gemv(const T*, const T*, const T*, T*, int, int, int, hipStream_t);
pgk_status wsgemm_nt(const bf16* a, int lda, const void* w, const bf16* wscale, bool fp8, void* c, const bf16* bias, int mode,
                     int splits, int M, int N, int K, hipStream_t st);
// (packed: W is the fragment-major bf16 copy of ops_pkgemm.hip instead of the row-major weight - the staged kernels' DMA
// instruction moves 16 rows x 32 k, which is one block of that layout)
pgk_status gemm256_bf16_nt(const bf16* A, const bf16* W, const bf16* bias, void* C, bool accum_f32, int M, int N, int K,
                           hipStream_t st, bool packed = false);
pgk_status gemm256_bf16_swiglu_nt(const bf16* A, const bf16* W, bf16* act, int M, int I, int K, hipStream_t st, bool packed = false);
bool gemm128s_ok(int M, int N, int K);    // ops_gemm256.hip: 128 x 128 tiles on the staged LDS-DMA pipeline (bf16, M > 128, K % 64 == 0, N % 8 == 0)
pgk_status gemm128s_bf16_nt(const bf16* A, const bf16* W, const bf16* bias, void* C, int mode, int splits, int M, int N, int K, hipStream_t st,
                            const QkvHeadArgs* heads = nullptr, bool packed = false);
// the 256 x 256 structure needs enough tiles to fill the chip and whole 128-byte K rows
// PGK_GEMM256 = 0 / 1 forces the choice (read per call: tests flip it to drive small shapes through both kernels); shared
// with the fp8 x fp8 GEMM (ops_fp8_gemm.hip)
bool want_gemm256(int M, int N) {
    const char* e = getenv("PGK_GEMM256");
    const int force = e ? atoi(e) : -1;
    if (force == 0) return false;
    if (force == 1) return true;
    return (long long)ceil_div(M, 256) * ceil_div(N, 256) >= 192;
}

enum BMode { B_NT = 0, B_NN = 1, B_NT_FP8 = 2, B_KN_FP8 = 3 };

template <class T, int BM, int BN, int MODE, int EPI>
// kps > 0 (B_NT only, EPI 2): split-K - workgroup z multiplies k in [z * kps, (z + 1) * kps) and stores its fp32 partial tile into
// slab z of Cv ([splits][M][N]); the consumer sums the slabs (the engine's RMSNorm kernel does, as for the skinny GEMMs).
__global__ __launch_bounds__(GEMM_THREADS) void gemm_mfma_kernel(const T* A, const void* Bv, const bf16* bscale,
                                                                const T* bias, void* Cv, int M, int N, int K, int kps) {
    constexpr int WM = BM / 2, WN = BN / 2, TM = WM / 16, TN = WN / 16;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;

    TileRegsK<BM> ra;
    TileRegsK<BN> rb_nt;
    TileRegsN<BN> rb_nn;
    TileRegsFp8NT<BN> rb_f8nt;
    TileRegsFp8KN<BN> rb_f8kn;

    const int kbeg = kps > 0 ? (int)blockIdx.z * kps : 0, kend = kps > 0 ? min(K, kbeg + kps) : K;
    auto load_tiles = [&](int k0) {
        ra.load(A, m0, M, k0, kend, K);
        if constexpr (MODE == B_NT) rb_nt.load((const T*)Bv, n0, N, k0, kend, K);
        else if constexpr (MODE == B_NN) rb_nn.load((const T*)Bv, n0, N, k0, K);
        else if constexpr (MODE == B_NT_FP8) rb_f8nt.load((const uint8_t*)Bv, bscale, n0, N, k0, K);
        else rb_f8kn.load((const uint8_t*)Bv, bscale, n0, N, k0, K);
    };
    auto store_tiles = [&](int buf) {
        char* as = gemm_tile_a<BM, BN>(smem, buf);
        char* bs = gemm_tile_b<BM, BN>(smem, buf);
        ra.store(as);
        if constexpr (MODE == B_NT) rb_nt.store(bs);
        else if constexpr (MODE == B_NN) rb_nn.store(bs);
        else if constexpr (MODE == B_NT_FP8) rb_f8nt.store(bs);
        else rb_f8kn.store(bs);
    };

    f32x4_t acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#include "gemm_tile_loop.hip.h"      // the main loop: acc += A . B^T over [kbeg, kend)

    // C/D map of v_mfma_f32_16x16x32: col = lane & 15, row = (lane >> 4) * 4 + reg
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int col = n0 + wn * WN + j * 16 + (lane & 15);
            if (col >= N) continue;
            const float b = bias ? to_f(bias[col]) : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wm * WM + i * 16 + (lane >> 4) * 4 + r;
                if (row >= M) continue;
                if constexpr (EPI == 0) reinterpret_cast<T*>(Cv)[(size_t)row * N + col] = from_f<T>(acc[i][j][r] + b);
                else if constexpr (EPI == 2) reinterpret_cast<float*>(Cv)[((size_t)blockIdx.z * M + row) * N + col] = acc[i][j][r];   // split-K slab
                else reinterpret_cast<float*>(Cv)[(size_t)row * N + col] += acc[i][j][r] + b;  // fp32 residual stream
            }
        }
}

// fp32 (and odd-shape) fallback: 64x64 tile, 16x16 threads x 4x4 outputs, LDS-staged.
template <class T, bool B_IS_NT>
__global__ __launch_bounds__(256) void gemm_simple_kernel(const T* A, const T* B, const T* bias, T* C, int M, int N, int K) {
    __shared__ float As[16][64 + 1];
    __shared__ float Bs[16][64 + 1];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    float acc[4][4] = {};
    for (int k0 = 0; k0 < K; k0 += 16) {
        for (int i = threadIdx.x; i < 64 * 16; i += 256) {
            const int r = i >> 4, k = i & 15;  // r: row in tile, k: k index
            const int gm = m0 + r, gn = n0 + r, gk = k0 + k;
            As[k][r] = (gm < M && gk < K) ? to_f(A[(size_t)gm * K + gk]) : 0.f;
            if (B_IS_NT) Bs[k][r] = (gn < N && gk < K) ? to_f(B[(size_t)gn * K + gk]) : 0.f;
        }
        if (!B_IS_NT) {
            for (int i = threadIdx.x; i < 64 * 16; i += 256) {
                const int k = i >> 6, c = i & 63;
                const int gk = k0 + k, gn = n0 + c;
                Bs[k][c] = (gk < K && gn < N) ? to_f(B[(size_t)gk * N + gn]) : 0.f;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { a[i] = As[k][ty * 4 + i]; b[i] = Bs[k][tx * 4 + i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gm = m0 + ty * 4 + i, gn = n0 + tx * 4 + j;
            if (gm < M && gn < N) C[(size_t)gm * N + gn] = from_f<T>(acc[i][j] + (bias ? to_f(bias[gn]) : 0.f));
        }
}

template <class T, int BM, int BN, int MODE, int EPI>
static pgk_status launch_mfma(const T* A, const void* B, const bf16* bscale, const T* bias, void* C, int M, int N, int K,
                              hipStream_t st, int splits = 1) {
    constexpr size_t LDS = gemm_tile_lds_bytes(BM, BN);
    dim3 grid(ceil_div(N, BN), ceil_div(M, BM), splits);
    const int kps = splits > 1 ? ceil_div(ceil_div(K, splits), GEMM_BK) * GEMM_BK : 0;
    return launch_dyn_lds<&gemm_mfma_kernel<T, BM, BN, MODE, EPI>>(grid, GEMM_THREADS, LDS, LDS > 48 * 1024, st, A, B, bscale, bias, C, M, N, K, kps);
}

// Tile choice: mfma_pick_tile (gemm_plan.h).
template <class T, int MODE, int EPI = 0>
static pgk_status dispatch_mfma(const T* A, const void* B, const bf16* bscale, const T* bias, void* C, int M, int N, int K,
                                hipStream_t st) {
    const MfmaTile tile = mfma_pick_tile(M, N, MODE == B_KN_FP8);      // gemm_plan.h
    const int bm = tile.bm, bn = tile.bn;
#define PGK_TILE(BM_, BN_) if (bm == BM_ && bn == BN_) return launch_mfma<T, BM_, BN_, MODE, EPI>(A, B, bscale, bias, C, M, N, K, st);
    PGK_TILE(128, 128) PGK_TILE(128, 64) PGK_TILE(128, 32)
    PGK_TILE(64, 128) PGK_TILE(64, 64) PGK_TILE(64, 32)
    PGK_TILE(32, 128) PGK_TILE(32, 64) PGK_TILE(32, 32)
#undef PGK_TILE
    return set_error(PGK_ERR_INVALID, "gemm: no tile for bm=%d bn=%d", bm, bn);
}

// fp8 codes [N,K] + 128x128 bf16 block scales -> bf16 [N,K] (exact: an e4m3 value times a bf16 scale rounds once)
__global__ __launch_bounds__(256) void dequant_fp8_blocks_kernel(const uint8_t* w8, const bf16* sw, bf16* out, int N, int K) {
    const size_t chunks = (size_t)N * K / 16, stride = (size_t)gridDim.x * blockDim.x;
    const int KB = K >> 7, cpr = K / 16;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < chunks; t += stride) {
        const int n = (int)(t / cpr), c = (int)(t % cpr);
        const uint4 raw = *reinterpret_cast<const uint4*>(w8 + (size_t)n * K + (size_t)c * 16);
        const float sc = to_f(sw[(size_t)(n >> 7) * KB + (c >> 3)]);
        uint4* o = reinterpret_cast<uint4*>(out + (size_t)n * K + (size_t)c * 16);
        o[0] = fp8x8_to_bf16x8(make_uint2(raw.x, raw.y), sc);
        o[1] = fp8x8_to_bf16x8(make_uint2(raw.z, raw.w), sc);
    }
}

// internal (engine prefill): N = hidden projections of a long prompt whose 128 x 128 tiles do not cover the chip (M = 2048,
// N = 1024: 128 tiles; the 64 x 64 tiles that do cover it run at 200-290 TFLOP/s) - the 128-tile kernel split along K into
// `splits` fp32 slabs [splits][M][N] that the next RMSNorm sums.  Returns the number of slabs through the argument; 1 = not used.
int engine_gemm_pick_splits(int M, int N, int K) {
    const long long tiles = (long long)ceil_div(M, 128) * ceil_div(N, 128);
    if (M <= 128 || tiles >= 192 || use_gemm256(M, N, K)) return 1;
    int s = (int)(256 / tiles);      // (512 workgroups - two per CU - measured the same to 3 %: S = 2048 4.86 vs 4.72 ms, S = 512 2.50 vs 2.52)
    if (s > 4) s = 4;
    while (s > 1 && (K / s < 512 || (gemm128s_ok(M, N, K) && K % (64 * s) != 0))) --s;
    return s < 1 ? 1 : s;
}
pgk_status engine_gemm_nt_slabs(const bf16* A, const void* W, float* slabs, int splits, int M, int N, int K, hipStream_t st, bool packed) {
    PGK_REQUIRE(splits >= 2 && K % 8 == 0, "engine_gemm_nt_slabs: splits=%d K=%d", splits, K);
    if (gemm128s_ok(M, N, K) && K % (64 * splits) == 0) return gemm128s_bf16_nt(A, (const bf16*)W, nullptr, slabs, 2, splits, M, N, K, st, nullptr, packed);
    PGK_REQUIRE(!packed, "engine_gemm_nt_slabs: M=%d N=%d K=%d splits=%d has no kernel that reads the fragment-major copy", M, N, K, splits);
    return launch_mfma<bf16, 128, 128, B_NT, 2>(A, W, nullptr, nullptr, slabs, M, N, K, st, splits);
}

// internal (engine prefill): bf16 A against a bf16 or fp8 (+128x128 bf16 block scales) weight W[N,K];
// either a bf16 result or an fp32 "+=" into the residual stream.
// the shapes whose kernels can read the fragment-major bf16 copy (engine_gemm_nt and friends with packed = true)
bool engine_gemm_packed_ok(int M, int N, int K) { return N % 16 == 0 && K % 64 == 0 && (use_gemm256(M, N, K) || gemm128s_ok(M, N, K)); }

pgk_status engine_gemm_nt(const bf16* A, const void* W, const bf16* wscale, bool fp8, void* C, bool accum_f32, int M,
                          int N, int K, hipStream_t st, bool packed) {
    if (packed) {
        PGK_REQUIRE(!fp8 && engine_gemm_packed_ok(M, N, K), "engine_gemm_nt: M=%d N=%d K=%d has no kernel that reads the fragment-major copy", M, N, K);
        if (use_gemm256(M, N, K)) return gemm256_bf16_nt(A, (const bf16*)W, nullptr, C, accum_f32, M, N, K, st, true);
        return gemm128s_bf16_nt(A, (const bf16*)W, nullptr, C, accum_f32 ? 1 : 0, 1, M, N, K, st, nullptr, true);
    }
    if (fp8 && w8a16_large_pick(M, N, K) == W8_DEQUANT_GEMM256) {
        // large w8a16 products: dequantise the weight once into a bf16 scratch (a ~10 % extra pass over memory) and run
        // the LDS-DMA bf16 kernel, instead of dequantising in the staging path of the 128-tile kernel (0.58 vs ~1 PFLOP/s)
        void* wb = nullptr;
        if (pgk_status r = pgk_malloc(&wb, (size_t)N * K * sizeof(bf16))) return r;
        const size_t chunks = (size_t)N * K / 16;
        dequant_fp8_blocks_kernel<<<(unsigned)(ceil_div((long long)chunks, 256) > 8192 ? 8192 : ceil_div((long long)chunks, 256)), 256, 0, st>>>(
            (const uint8_t*)W, wscale, (bf16*)wb, N, K);
        const pgk_status r = gemm256_bf16_nt(A, (const bf16*)wb, nullptr, C, accum_f32, M, N, K, st);
        pgk_free(wb);   // stream-ordered reuse
        return r;
    }
    if (fp8) {
        if (accum_f32) return dispatch_mfma<bf16, B_NT_FP8, 1>(A, W, wscale, nullptr, C, M, N, K, st);
        return dispatch_mfma<bf16, B_NT_FP8, 0>(A, W, wscale, nullptr, C, M, N, K, st);
    }
    if (use_gemm256(M, N, K)) return gemm256_bf16_nt(A, (const bf16*)W, nullptr, C, accum_f32, M, N, K, st);
    if (gemm128s_ok(M, N, K)) return gemm128s_bf16_nt(A, (const bf16*)W, nullptr, C, accum_f32 ? 1 : 0, 1, M, N, K, st);
    if (accum_f32) return dispatch_mfma<bf16, B_NT, 1>(A, W, nullptr, nullptr, C, M, N, K, st);
    return dispatch_mfma<bf16, B_NT, 0>(A, W, nullptr, nullptr, C, M, N, K, st);
}

// internal (engine prefill, bf16 weights, head_dim 128): the QKV projection with per-head RMSNorm + RoPE + KV-cache write as its
// epilogue (QkvHeadArgs) - on the 128-tile kernel, whose tile columns are whole heads; where engine_gemm_nt would pick the
// 256-tile kernel the separate pass stays
bool engine_gemm_qkv_heads_ok(int M, int N, int K) { return N % 128 == 0 && gemm128s_ok(M, N, K) && !use_gemm256(M, N, K); }
pgk_status engine_gemm_qkv_heads_nt(const bf16* A, const bf16* W, bf16* qkv, int M, int N, int K, const QkvHeadArgs& hd, hipStream_t st, bool packed) {
    PGK_REQUIRE(engine_gemm_qkv_heads_ok(M, N, K), "engine_gemm_qkv_heads: M=%d N=%d K=%d outside the fused kernel's shapes", M, N, K);
    return gemm128s_bf16_nt(A, W, nullptr, qkv, 3, 1, M, N, K, st, &hd, packed);
}

// internal (engine prefill): act[M][I] = bf16(silu(A . Wg^T) * (A . Wu^T)) on the fused [2 I, K] gate / up weight (bf16, or fp8 with
// block scales: dequantised once into a bf16 scratch as in engine_gemm_nt), SwiGLU in the 256-tile kernel's epilogue - the
// [M][2 I] intermediate never goes to HBM.  Only where engine_gemm_nt would pick the 256-tile kernel anyway.
// (below 192 tiles of 256 x 256, bf16 weights: the same epilogue on the 128-tile kernel, 64 gate + 64 up rows per tile)
bool engine_gemm_swiglu_ok(int M, int I, int K, bool fp8) {
    if (I % 128 == 0 && use_gemm256(M, 2 * I, K) && (!fp8 || K % 128 == 0)) return true;
    return !fp8 && I % 64 == 0 && gemm128s_ok(M, I, K);
}
pgk_status engine_gemm_swiglu_nt(const bf16* A, const void* W, const bf16* wscale, bool fp8, bf16* act, int M, int I, int K, hipStream_t st, bool packed) {
    PGK_REQUIRE(engine_gemm_swiglu_ok(M, I, K, fp8) && !(packed && fp8), "engine_gemm_swiglu: M=%d I=%d K=%d outside the fused kernel's shapes", M, I, K);
    if (!(I % 128 == 0 && use_gemm256(M, 2 * I, K))) return gemm128s_bf16_nt(A, (const bf16*)W, nullptr, act, 4, 1, M, I, K, st, nullptr, packed);
    if (!fp8) return gemm256_bf16_swiglu_nt(A, (const bf16*)W, act, M, I, K, st, packed);
    void* wb = nullptr;
    if (pgk_status r = pgk_malloc(&wb, (size_t)2 * I * K * sizeof(bf16))) return r;
    const size_t chunks = (size_t)2 * I * K / 16;
    dequant_fp8_blocks_kernel<<<(unsigned)(ceil_div((long long)chunks, 256) > 8192 ? 8192 : ceil_div((long long)chunks, 256)), 256, 0, st>>>(
        (const uint8_t*)W, wscale, (bf16*)wb, 2 * I, K);
    const pgk_status r = gemm256_bf16_swiglu_nt(A, (const bf16*)wb, act, M, I, K, st);
    pgk_free(wb);   // stream-ordered reuse
    return r;
}

}  // namespace pgk

using namespace pgk;

extern "C" {

pgk_status pgk_gemm_nt(const void* a, const void* w, const void* bias, void* c, int m, int n, int k, pgk_dtype dt,
                       pgk_stream s) {
    PGK_REQUIRE(a && w && c, "pgk_gemm_nt: null pointer");
    PGK_REQUIRE(m >= 0 && n > 0 && k > 0, "pgk_gemm_nt: bad shape M=%d N=%d K=%d", m, n, k);
    if (!m) return PGK_OK;
    hipStream_t st = resolve_stream(s);
    switch (gemm_nt_pick(m, n, k, dt, aligned16(a) && aligned16(w))) {      // gemm_plan.h
        case NT_GEMV:
            PGK_DISPATCH_FLOAT(dt, "pgk_gemm_nt", return (launch_gemv<T>((const T*)a, (const T*)w, (const T*)bias, (T*)c, m, k, n, st)));
            return PGK_OK;
        case NT_SIMPLE: {
            dim3 grid(ceil_div(n, 64), ceil_div(m, 64));
            PGK_DISPATCH_FLOAT(dt, "pgk_gemm_nt", (gemm_simple_kernel<T, true><<<grid, 256, 0, st>>>((const T*)a, (const T*)w, (const T*)bias, (T*)c, m, n, k)));
            PGK_LAUNCH_CHECK();
            return PGK_OK;
        }
        case NT_WSGEMM: return wsgemm_nt((const bf16*)a, k, w, nullptr, false, c, (const bf16*)bias, 0, 1, m, n, k, st);
        case NT_GEMM256: return gemm256_bf16_nt((const bf16*)a, (const bf16*)w, (const bf16*)bias, c, false, m, n, k, st);
        case NT_GEMM128S: return gemm128s_bf16_nt((const bf16*)a, (const bf16*)w, (const bf16*)bias, c, 0, 1, m, n, k, st);
        case NT_MFMA: break;
    }
    if (dt == PGK_BF16) return dispatch_mfma<bf16, B_NT>((const bf16*)a, w, nullptr, (const bf16*)bias, (bf16*)c, m, n, k, st);
    if (dt == PGK_F16) return dispatch_mfma<f16, B_NT>((const f16*)a, w, nullptr, (const f16*)bias, (f16*)c, m, n, k, st);
    return set_error(PGK_ERR_INVALID, "pgk_gemm_nt: unsupported dtype %d", (int)dt);
}

pgk_status pgk_gemm_nn(const void* a, const void* b, void* c, int m, int n, int k, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(a && b && c, "pgk_gemm_nn: null pointer");
    PGK_REQUIRE(m >= 0 && n > 0 && k > 0, "pgk_gemm_nn: bad shape M=%d N=%d K=%d", m, n, k);
    if (!m) return PGK_OK;
    hipStream_t st = resolve_stream(s);
    if (gemm_nn_pick(n, k, dt, aligned16(a) && aligned16(b)) == NN_SIMPLE) {      // gemm_plan.h
        dim3 grid(ceil_div(n, 64), ceil_div(m, 64));
        PGK_DISPATCH_FLOAT(dt, "pgk_gemm_nn", (gemm_simple_kernel<T, false><<<grid, 256, 0, st>>>((const T*)a, (const T*)b, nullptr, (T*)c, m, n, k)));
        PGK_LAUNCH_CHECK();
        return PGK_OK;
    }
    if (dt == PGK_BF16) return dispatch_mfma<bf16, B_NN>((const bf16*)a, b, nullptr, nullptr, (bf16*)c, m, n, k, st);
    if (dt == PGK_F16) return dispatch_mfma<f16, B_NN>((const f16*)a, b, nullptr, nullptr, (f16*)c, m, n, k, st);
    return set_error(PGK_ERR_INVALID, "pgk_gemm_nn: unsupported dtype %d", (int)dt);
}

pgk_status pgk_w8a16_gemm_nk(const void* a, const uint8_t* w_nk, const void* scale, void* c, int m, int n, int k,
                             pgk_stream s) {
    PGK_REQUIRE(a && w_nk && scale && c, "pgk_w8a16_gemm_nk: null pointer");
    PGK_REQUIRE(m >= 0 && n > 0 && k > 0, "pgk_w8a16_gemm_nk: bad shape M=%d N=%d K=%d", m, n, k);
    PGK_REQUIRE(k % 128 == 0 && n % 128 == 0, "pgk_w8a16_gemm_nk: K=%d, N=%d must be multiples of the 128x128 scale block", k, n);
    PGK_REQUIRE(aligned16(a) && aligned16(w_nk), "pgk_w8a16_gemm_nk: operands must be 16-byte aligned");
    if (!m) return PGK_OK;
    if (w8a16_nk_pick(m, n, k) == W8_WSGEMM)      // gemm_plan.h; engine_gemm_nt takes W8_DEQUANT_GEMM256 / W8_MFMA by the same function
        return wsgemm_nt((const bf16*)a, k, w_nk, (const bf16*)scale, true, c, nullptr, 0, 1, m, n, k, resolve_stream(s));
    return engine_gemm_nt((const bf16*)a, w_nk, (const bf16*)scale, true, c, false, m, n, k, resolve_stream(s), false);
}

pgk_status pgk_w8a16_gemm_kn(const void* a, const uint8_t* b_kn, const void* scale, void* c, int m, int n, int k,
                             pgk_stream s) {
    PGK_REQUIRE(a && b_kn && scale && c, "pgk_w8a16_gemm_kn: null pointer");
    PGK_REQUIRE(m >= 0 && n > 0 && k > 0, "pgk_w8a16_gemm_kn: bad shape M=%d N=%d K=%d", m, n, k);
    PGK_REQUIRE(k % 128 == 0 && n % 128 == 0, "pgk_w8a16_gemm_kn: K=%d, N=%d must be multiples of the 128x128 scale block", k, n);
    PGK_REQUIRE(aligned16(a) && aligned16(b_kn), "pgk_w8a16_gemm_kn: operands must be 16-byte aligned");
    if (!m) return PGK_OK;
    return dispatch_mfma<bf16, B_KN_FP8>((const bf16*)a, b_kn, (const bf16*)scale, nullptr, (bf16*)c, m, n, k, resolve_stream(s));
}

// The kernel a call of this shape takes, as text (tests assert it; see DESIGN.md "GEMM dispatch leaves").  Built from the
// decision functions of gemm_plan.h that the entry points above and their launchers switch on; needs no device.
// NULL (and pgk_last_error) for an op name, dtype or shape that the entry point itself rejects.
const char* pgk_gemm_plan(const char* op, int m, int n, int k, pgk_dtype dt, int aligned) {
    static thread_local char buf[96];
    const auto fail = [](const char* why, const char* op_, int m_, int n_, int k_, int dt_) -> const char* {
        set_error(PGK_ERR_INVALID, "pgk_gemm_plan: %s (op=%s M=%d N=%d K=%d dtype=%d)", why, op_ ? op_ : "NULL", m_, n_, k_, dt_);
        return nullptr;
    };
    if (!op) return fail("null op", op, m, n, k, (int)dt);
    if (m < 1 || n < 1 || k < 1) return fail("bad shape", op, m, n, k, (int)dt);
    const std::string o(op);
    const bool al = aligned != 0;
    const auto gemm256 = [&](const char* prefix) -> const char* {
        static const char* const names[] = {"gemm256s", "gemm256s_n192", "gemm256_lockstep"};
        snprintf(buf, sizeof buf, "%s%s", prefix, names[gemm256_pick(m, n, false, false)]);
        return buf;
    };
    const auto mfma = [&](const char* mode, bool kn) -> const char* {
        const MfmaTile t = mfma_pick_tile(m, n, kn);
        snprintf(buf, sizeof buf, "mfma_%dx%d_%s", t.bm, t.bn, mode);
        return buf;
    };
    const auto wsgemm = [&](bool fp8) -> const char* {
        snprintf(buf, sizeof buf, "wsgemm_mt%d%s", wsgemm_pick_mt(m), fp8 ? "_fp8" : "");
        return buf;
    };
    if (o == "nt" || o == "nn") {
        if (!is_float_dtype(dt)) return fail("dtype must be float32, float16 or bfloat16", op, m, n, k, (int)dt);
        if (o == "nn") {
            if (gemm_nn_pick(n, k, dt, al) == NN_SIMPLE) return "simple_nn";
            return mfma("B_NN", false);
        }
        switch (gemm_nt_pick(m, n, k, dt, al)) {
            case NT_GEMV:
                if (gemv_pick(m, k, dtype_size(dt), al) == GEMV_GENERIC) return "gemv_generic";
                snprintf(buf, sizeof buf, "gemv_fast_m%d", m);
                return buf;
            case NT_SIMPLE: return "simple_nt";
            case NT_WSGEMM: return wsgemm(false);
            case NT_GEMM256: return gemm256("");
            case NT_GEMM128S: return "gemm128s";
            case NT_MFMA: return mfma("B_NT", false);
        }
        return fail("no kernel", op, m, n, k, (int)dt);
    }
    // the fp8 entry points: bf16 activations / output, 16-byte aligned operands and whole 128 x 128 scale blocks by contract
    if (dt != PGK_BF16) return fail("the fp8 entry points are bfloat16", op, m, n, k, (int)dt);
    if (!al) return fail("the fp8 entry points need 16-byte aligned operands", op, m, n, k, (int)dt);
    if (o == "fp8_nt") {
        if (k % 128) return fail("K must be a multiple of 128", op, m, n, k, (int)dt);
        return gemm_fp8_pick(m, n) == FP8_TILE256 ? "fp8_256" : "fp8_128";
    }
    if (k % 128 || n % 128) return fail("K and N must be multiples of the 128 x 128 scale block", op, m, n, k, (int)dt);
    if (o == "w8a16_nk") {
        switch (w8a16_nk_pick(m, n, k)) {
            case W8_WSGEMM: return wsgemm(true);
            case W8_DEQUANT_GEMM256: return gemm256("dequant+");
            case W8_MFMA: return mfma("B_NT_FP8", false);
        }
    }
    if (o == "w8a16_kn") return mfma("B_KN_FP8", true);
    if (o == "gemv_fp8") {
        if ((size_t)gemv_fp8_pass_rows(m, 0) * k * 2 > 64 * 1024) return fail("K too large for the rows of one pass", op, m, n, k, (int)dt);
        const int full = m / 8, rest = m % 8;       // passes of gemv_fp8_pass_rows: `full` of 8 rows, then the rest
        if (m <= 8) snprintf(buf, sizeof buf, "gemv_fp8_m%d", m);
        else if (rest) snprintf(buf, sizeof buf, "gemv_fp8_m8x%d+m%d", full, rest);
        else snprintf(buf, sizeof buf, "gemv_fp8_m8x%d", full);
        return buf;
    }
    return fail("op must be one of nt, nn, w8a16_nk, w8a16_kn, gemv_fp8, fp8_nt", op, m, n, k, (int)dt);
}

}  // extern "C"
