// Flash-attention prefill with an fp8 first product (sdpa_causal_fp8; bf16 in / out, head_dim 128) for gfx950.
//
//   Q, K -> e4m3 codes with ONE power-of-two scale per head (UE8M0 byte e + 127; reference
//           quantize_to_fp8_e4m3_per_head_kernel, native/ops/nn/attention/flash_attention_3_fp8_sm120.cuh:475-547):
//           a = max |X_h|, e = 0 for a == 0, else the smallest integer with 448 * 2^e >= a clamped to [-127, 127],
//           code = e4m3(X * 2^-e) RNE.  e is taken from a's bf16 exponent and mantissa fields (448 = 1.75 * 2^8), not
//           from log2f, and the multiply by a power of two is exact: codes and scale bytes are reproducible bit for bit.
//   s[i][j] = scale * 2^(eq + ek) * sum_d T[qc[i][d]] * T[kc[j][d]]      (fp8 products, fp32 sums)
//   out     = softmax_j(s + causal mask) . V                            (fp32 softmax, V and P in bf16)
//
// The kernel is flash_core.hip.h's tile walk - flash_fwd_kernel's (ops_flash.hip) - around another first product:
// S^T[32 kv][32 q] = K . Q^T is two v_mfma_f32_32x32x64_f8f6f4 steps over d (e4m3 operands, twice the bf16 rate per clock)
// instead of eight bf16 steps.
// K codes are the A operand, read from an fp8 LDS image (128-byte rows, 8 KiB per 64-position tile: 48 KiB per workgroup
// with the V^T tiles instead of 64); Q codes stay in registers as the B operand.  Both operands give lane l the SAME 32
// bytes of their row - d = 64 s + 32 (l >> 5) .. + 31 of row l & 31 - so the contraction pairs matching d whatever order
// the hardware walks the 32 bytes in (as gemm_fp8_kernel, ops_fp8_gemm.hip; pinned by the exact-integer GPU test).  The
// C/D layout depends on the shape only, so the transposed softmax and the P packing are the shared ones, and the
// second product O^T += V^T . P^T stays on v_mfma_f32_32x32x16_bf16 with the same V^T pre-pass and image.
// The factor 2^(eq + ek) is NOT put in the instruction's e8m0 scale operands: it is folded with scale * log2(e) into one
// fp32 constant per head, applied inside the exp2 argument as an FMA that replaces the subtraction of the running maximum
// (no extra instruction; the maximum itself is taken on the raw sums, the constant being positive).  The softmax scale
// cannot be multiplied into Q before quantisation as the bf16 kernel does: that would change the codes.

#include "flash_core.hip.h"

namespace pgk {

typedef int i32x8_f8 __attribute__((ext_vector_type(8)));

struct Fp8HeadSrc {          // one tensor [heads][rows][128] bf16 with (head, row) element strides
    const bf16* x;
    uint8_t* codes;          // [heads][rows][128]
    uint8_t* scale_bytes;    // [heads]
    uint32_t* amax;          // [heads] bf16 magnitude bits of the head's absmax (zeroed before the absmax pass)
    int heads, rows;
    long long sh, ss;
};

// smallest e with 448 * 2^e >= a (a > 0 given as bf16 magnitude bits: 448 = 1.75 * 2^8 has exponent field 135, mantissa 96)
__device__ __forceinline__ int fp8_head_exp(uint32_t a) {
    if (a == 0) return 0;
    const int e = (int)(a >> 7) - 135 + ((a & 127u) > 96u ? 1 : 0);
    return max(-127, min(127, e));
}

// grid (blocks, heads of a + heads of b): the maximum of a head goes through a vector atomic max on the magnitude bits
__global__ __launch_bounds__(256) void fp8_head_absmax_kernel(Fp8HeadSrc a, Fp8HeadSrc b) {
    const bool second = (int)blockIdx.y >= a.heads;
    const Fp8HeadSrc t = second ? b : a;
    const int head = second ? blockIdx.y - a.heads : blockIdx.y;
    const bf16* xh = t.x + (size_t)head * t.sh;
    const long long nchunk = (long long)t.rows * 16;
    uint32_t m = 0;
    for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < nchunk; c += (long long)gridDim.x * 256) {
        const uint4 v = *reinterpret_cast<const uint4*>(xh + (c >> 4) * t.ss + (c & 15) * 8);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) m = max(m, max(w[j] & 0x7FFFu, (w[j] >> 16) & 0x7FFFu));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off, 64));
    if ((threadIdx.x & 63) == 0 && m != 0) atomicMax(t.amax + head, m);
}

__global__ __launch_bounds__(256) void fp8_head_codes_kernel(Fp8HeadSrc a, Fp8HeadSrc b) {
    const bool second = (int)blockIdx.y >= a.heads;
    const Fp8HeadSrc t = second ? b : a;
    const int head = second ? blockIdx.y - a.heads : blockIdx.y;
    const int e = fp8_head_exp(t.amax[head]);
    if (blockIdx.x == 0 && threadIdx.x == 0) t.scale_bytes[head] = (uint8_t)(e + 127);
    // 2^-e: exponent field 127 - e, and the subnormal 2^-127 for e = 127
    const float mul = __uint_as_float(e < 127 ? (uint32_t)(127 - e) << 23 : 0x00400000u);
    const bf16* xh = t.x + (size_t)head * t.sh;
    uint8_t* ch = t.codes + (size_t)head * t.rows * 128;
    const long long nchunk = (long long)t.rows * 16;
    for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < nchunk; c += (long long)gridDim.x * 256) {
        Vec<bf16> v;
        v.load(xh + (c >> 4) * t.ss + (c & 15) * 8);
        float f[8];
        v.to_float(f);
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = fminf(fmaxf(f[j] * mul, -448.0f), 448.0f);    // satfinite (|x 2^-e| <= 448 for finite x anyway)
        *reinterpret_cast<uint2*>(ch + c * 8) = make_uint2(pack_fp8x4(f[0], f[1], f[2], f[3]), pack_fp8x4(f[4], f[5], f[6], f[7]));
    }
}

// both passes for up to two tensors; amax of both must be zeroed by the caller's memset on the same stream
static pgk_status fp8_quantize_heads(const Fp8HeadSrc& a, const Fp8HeadSrc& b, hipStream_t st) {
    const long long chunks = 16LL * (a.rows > b.rows || b.heads == 0 ? a.rows : b.rows);
    const int blocks = (int)min(64LL, (chunks + 1023) / 1024);      // four 16-byte chunks per thread and more on long inputs
    const dim3 grid(blocks, a.heads + b.heads);
    fp8_head_absmax_kernel<<<grid, 256, 0, st>>>(a, b);
    fp8_head_codes_kernel<<<grid, 256, 0, st>>>(a, b);
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

// K image: [64 kv][128] e4m3 = 128-byte rows, 16-byte chunk c (0..7) of row r at r*128 + ((c ^ ((r >> 1) & 7)) << 4): the 16
// rows a quarter-wave reads at one c, and the 2 rows x 8 chunks it stages, each fall on 64 different banks (by address
// arithmetic; no LDS-conflict counter was collected)
__device__ __forceinline__ int fl8_k_off(int r, int c) { return r * 128 + ((c ^ ((r >> 1) & 7)) << 4); }

constexpr int FL8_K_BYTES = 64 * 128, FL8_V_BYTES = 128 * 128;
constexpr size_t FL8_LDS = 2 * (size_t)FL8_K_BYTES + 2 * (size_t)FL8_V_BYTES;

// q8 [Hq][q_len][128], k8 [Hkv][kv_len][128] e4m3 codes; qsb / ksb their UE8M0 head scale bytes; vt as flash_fwd_kernel
__global__ __launch_bounds__(FL_THREADS, 2) void flash_fwd_fp8_kernel(const uint8_t* q8, const uint8_t* k8, const uint8_t* qsb, const uint8_t* ksb,
                                                                  const bf16* vt, bf16* out, int hq, int hkv, int q_len, int kv_len,
                                                                  int kv_pad, float scale_log2e, FlashStrides sd, FlashSplit sp) {
    typedef bf16 T;
    constexpr int D = 128, DT = D / 32;
    extern __shared__ __attribute__((aligned(16))) char fl8_smem[];   // K[2] | V^T[2]
    auto Ks = [&](int buf) -> char* { return fl8_smem + buf * FL8_K_BYTES; };

    const int tid = threadIdx.x, lane = tid & 63, ql = lane & 31, h = lane >> 5;
    const FlashWork wk = flash_work(hq, hkv, q_len, sp.nsplit, kv_len - q_len);
    const int head = wk.head, kvh = wk.kvh, qw0 = wk.qw0;
    const uint8_t* kh = k8 + (size_t)kvh * kv_len * D;
    // raw fp8 sum -> score in the exp2 domain: scale * log2(e) * 2^(eq + ek)
    // clamped to the normal fp32 range: an underflow to 0 would turn a masked score (-inf * 0) into a NaN, an overflow a zero sum
    // (0 * inf); heads that small or large (eq + ek beyond about +-125) get scores scaled by the clamped constant instead
    const float cf = fminf(fmaxf(ldexpf(scale_log2e, (int)qsb[head] + (int)ksb[kvh] - 254), 1.17549435e-38f), 3.40282347e+38f);

    // Q^T fragments (B operand): lane = query column, step s holds d = 64 s + 32 h .. + 31
    i32x8_f8 qf0, qf1;
    {
        const uint8_t* qrow = q8 + ((size_t)head * q_len + min(qw0 + ql, q_len - 1)) * D + 32 * h;
        const uint4 a0 = *reinterpret_cast<const uint4*>(qrow), a1 = *reinterpret_cast<const uint4*>(qrow + 16);
        const uint4 b0 = *reinterpret_cast<const uint4*>(qrow + 64), b1 = *reinterpret_cast<const uint4*>(qrow + 80);
        qf0 = i32x8_f8{(int)a0.x, (int)a0.y, (int)a0.z, (int)a0.w, (int)a1.x, (int)a1.y, (int)a1.z, (int)a1.w};
        qf1 = i32x8_f8{(int)b0.x, (int)b0.y, (int)b0.z, (int)b0.w, (int)b1.x, (int)b1.y, (int)b1.z, (int)b1.w};
    }
    f32x16_fl o[DT];
#pragma unroll
    for (int i = 0; i < DT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;    // running max (scaled, log2 domain) and this lane's half of the row sum

    // K staging in named registers, as FlashVStage (flash_core.hip.h): chunk i of this thread is row kr + 32 i, 16-byte chunk kc - a
    // whole tile is 8 KiB of contiguous codes, chunk index = tid + 256 i
    uint4 rk0, rk1;
    const int kr = tid >> 3, kc = tid & 7;
    FlashVStage<T, DT> vst(tid, kv_pad);
    auto load_k = [&](int t) {
        const int kv0 = t * FL_BKV;
        if (kv0 + FL_BKV <= kv_len) {      // wave-uniform
            const uint8_t* kt = kh + (size_t)kv0 * D + tid * 16;
            rk0 = *reinterpret_cast<const uint4*>(kt);
            rk1 = *reinterpret_cast<const uint4*>(kt + 4096);
        } else {                           // the ragged last tile clamps its rows
            rk0 = *reinterpret_cast<const uint4*>(kh + (size_t)min(kv0 + kr, kv_len - 1) * D + kc * 16);
            rk1 = *reinterpret_cast<const uint4*>(kh + (size_t)min(kv0 + kr + 32, kv_len - 1) * D + kc * 16);
        }
    };
    auto store_k = [&](int buf) {
        char* kb = Ks(buf);
        *reinterpret_cast<uint4*>(kb + fl8_k_off(kr, kc)) = rk0;
        *reinterpret_cast<uint4*>(kb + fl8_k_off(kr + 32, kc)) = rk1;
    };
    auto k_frag = [&](int buf, int row, int s) -> i32x8_f8 {
        const uint4 lo = *reinterpret_cast<const uint4*>(Ks(buf) + fl8_k_off(row, 4 * s + 2 * h));
        const uint4 hi = *reinterpret_cast<const uint4*>(Ks(buf) + fl8_k_off(row, 4 * s + 2 * h + 1));
        return i32x8_f8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
    };
    // S^T = K . Q^T of one tile (raw fp8 sums): two 32-kv sub-tiles (rows = positions, column = this lane's query), two
    // 64-d steps each; cbsz = blgp = 0 selects e4m3 for both operands, scale operands 0 = the instruction's unscaled form
    auto qk = [&](int buf, int, f32x16_fl& s0, f32x16_fl& s1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { s0[r] = 0.f; s1[r] = 0.f; }
        const i32x8_f8 a00 = k_frag(buf, ql, 0), a10 = k_frag(buf, 32 + ql, 0);
        const i32x8_f8 a01 = k_frag(buf, ql, 1), a11 = k_frag(buf, 32 + ql, 1);
        s0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a00, qf0, s0, 0, 0, 0, 0, 0, 0);
        s1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a10, qf0, s1, 0, 0, 0, 0, 0, 0);
        s0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a01, qf1, s0, 0, 0, 0, 0, 0, 0);
        s1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a11, qf1, s1, 0, 0, 0, 0, 0, 0);
    };
    auto retire_q = [&] {      // why: flash_walk
#pragma unroll
        for (int j = 0; j < 8; ++j) asm volatile("" ::"v"(qf0[j]), "v"(qf1[j]));
    };
    flash_walk<T, DT, true>(wk, vst, vt + (size_t)kvh * D * kv_pad, q_len, kv_len, sp.nsplit, ql, h, fl8_smem + 2 * FL8_K_BYTES, o, m_run, l_run, cf, load_k,
                            store_k, retire_q, qk);

    float inv;
    const float l_tot = flash_row_sum(l_run, inv);
    flash_store_row<T, DT>(wk, o, m_run, l_tot, inv, ql, h, out, hq, q_len, sd, sp);
}

static pgk_status flash_fp8_launch(const bf16* q, const bf16* k, const bf16* v, bf16* out, int hq, int hkv, int q_len, int kv_len, float scale,
                                   const FlashStrides& sd, hipStream_t st) {
    constexpr int D = 128;
    auto up256 = [](size_t n) { return (n + 255) & ~(size_t)255; };
    // behind the plan's regions: Q codes | K codes | head absmax | head scale bytes
    const size_t q8_bytes = up256((size_t)hq * q_len * D), k8_bytes = up256((size_t)hkv * kv_len * D);
    const size_t am_bytes = up256((size_t)(hq + hkv) * sizeof(uint32_t)), sb_bytes = up256((size_t)(hq + hkv));
    // the split is the bf16 kernel's choice: same occupancy, same tile walk
    const FlashPlan p = flash_plan(hq, hkv, q_len, kv_len, kv_len, D, device_cu_count(), q8_bytes + k8_bytes + am_bytes + sb_bytes);
    void* ws = nullptr;
    if (pgk_status r = pgk_malloc(&ws, p.bytes)) return r;
    const FlashSplit sp = flash_split(p, ws);
    uint8_t* q8 = (uint8_t*)ws + p.extra_off;
    uint8_t* k8 = q8 + q8_bytes;
    uint32_t* amax = (uint32_t*)(k8 + k8_bytes);
    uint8_t* sb = k8 + k8_bytes + am_bytes;
    hipError_t e = hipMemsetAsync(amax, 0, (size_t)(hq + hkv) * sizeof(uint32_t), st);
    pgk_status r = PGK_OK;
    if (e == hipSuccess) {
        const Fp8HeadSrc qs{q, q8, sb, amax, hq, q_len, sd.qh, sd.qs}, ks{k, k8, sb + hq, amax + hq, hkv, kv_len, sd.kh, sd.ks};
        r = fp8_quantize_heads(qs, ks, st);
    }
    if (e == hipSuccess && r == PGK_OK) {
        e = flash_run<bf16, D>(p, ws, sp, v, out, hq, hkv, q_len, kv_len, sd, st, [&](int grid, const bf16* vt) {
            flash_fwd_fp8_kernel<<<grid, FL_THREADS, FL8_LDS, st>>>(q8, k8, sb, sb + hq, vt, out, hq, hkv, q_len, kv_len, p.kv_pad,
                                                                   scale * 1.4426950408889634f, sd, sp);
        });
    }
    pgk_free(ws);   // stream-ordered reuse: later work on this stream runs after the kernels above
    if (r != PGK_OK) return r;
    PGK_CHECK_HIP(e);
    return PGK_OK;
}

}  // namespace pgk

extern "C" {

pgk_status pgk_sdpa_causal_fp8(const void* q, const void* k, const void* v, void* out, int hq, int hkv, int q_len, int kv_len, int d,
                               float scale, int64_t q_stride_h, int64_t q_stride_s, int64_t kv_stride_h, int64_t kv_stride_s,
                               int64_t o_stride_h, int64_t o_stride_s, pgk_dtype dt, pgk_stream s) {
    using namespace pgk;
    PGK_REQUIRE(q && k && v && out, "pgk_sdpa_causal_fp8: null pointer");
    PGK_REQUIRE(dt == PGK_BF16, "pgk_sdpa_causal_fp8: bfloat16 only (dtype %d)", (int)dt);
    PGK_REQUIRE(d == 128, "pgk_sdpa_causal_fp8: head_dim must be 128 (got %d)", d);
    PGK_REQUIRE(hq > 0 && hkv > 0 && hq % hkv == 0, "pgk_sdpa_causal_fp8: n_heads mismatch (Hq=%d, Hkv=%d)", hq, hkv);
    PGK_REQUIRE(q_len > 0 && kv_len > 0, "pgk_sdpa_causal_fp8: bad shape q_len=%d kv_len=%d", q_len, kv_len);
    PGK_REQUIRE(kv_len >= q_len, "pgk_sdpa_causal_fp8: kv_len %d < q_len %d", kv_len, q_len);
    PGK_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out) &&
                    ((q_stride_h | q_stride_s | kv_stride_h | kv_stride_s | o_stride_h | o_stride_s) & 7) == 0,
                "pgk_sdpa_causal_fp8: pointers must be 16-byte aligned and strides multiples of 8 elements");
    if (scale <= 0.f) scale = 1.0f / sqrtf((float)d);
    const FlashStrides sd{q_stride_h, q_stride_s, kv_stride_h, kv_stride_s, o_stride_h, o_stride_s};
    return flash_fp8_launch((const bf16*)q, (const bf16*)k, (const bf16*)v, (bf16*)out, hq, hkv, q_len, kv_len, scale, sd, resolve_stream(s));
}

pgk_status pgk_quantize_fp8_per_head(const void* x, uint8_t* codes, uint8_t* scale_bytes, int heads, int rows, int d, int64_t stride_h,
                                     int64_t stride_s, pgk_dtype dt, pgk_stream s) {
    using namespace pgk;
    PGK_REQUIRE(x && codes && scale_bytes, "pgk_quantize_fp8_per_head: null pointer");
    PGK_REQUIRE(dt == PGK_BF16, "pgk_quantize_fp8_per_head: bfloat16 only (dtype %d)", (int)dt);
    PGK_REQUIRE(d == 128, "pgk_quantize_fp8_per_head: head_dim must be 128 (got %d)", d);
    PGK_REQUIRE(heads > 0 && rows > 0, "pgk_quantize_fp8_per_head: bad shape heads=%d rows=%d", heads, rows);
    PGK_REQUIRE(aligned16(x) && (reinterpret_cast<uintptr_t>(codes) & 7u) == 0 && ((stride_h | stride_s) & 7) == 0,
                "pgk_quantize_fp8_per_head: x must be 16-byte aligned, codes 8-byte aligned, strides multiples of 8 elements");
    hipStream_t st = resolve_stream(s);
    void* ws = nullptr;
    const size_t am_bytes = (size_t)heads * sizeof(uint32_t);
    if (pgk_status r = pgk_malloc(&ws, am_bytes)) return r;
    hipError_t e = hipMemsetAsync(ws, 0, am_bytes, st);
    pgk_status r = PGK_OK;
    if (e == hipSuccess) {
        const Fp8HeadSrc a{(const bf16*)x, codes, scale_bytes, (uint32_t*)ws, heads, rows, stride_h, stride_s};
        r = fp8_quantize_heads(a, Fp8HeadSrc{nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0}, st);
    }
    pgk_free(ws);
    if (r != PGK_OK) return r;
    PGK_CHECK_HIP(e);
    return PGK_OK;
}

}  // extern "C"
