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
// The kernel is flash_fwd_kernel (ops_flash.hip) with its first product replaced: S^T[32 kv][32 q] = K . Q^T is two
// v_mfma_f32_32x32x64_f8f6f4 steps over d (e4m3 operands, twice the bf16 rate per clock) instead of eight bf16 steps.
// K codes are the A operand, read from an fp8 LDS image (128-byte rows, 8 KiB per 64-position tile: 48 KiB per workgroup
// with the V^T tiles instead of 64); Q codes stay in registers as the B operand.  Both operands give lane l the SAME 32
// bytes of their row - d = 64 s + 32 (l >> 5) .. + 31 of row l & 31 - so the contraction pairs matching d whatever order
// the hardware walks the 32 bytes in (as gemm_fp8_kernel, ops_fp8_gemm.hip; pinned by the exact-integer GPU test).  The
// C/D layout depends on the shape only, so the transposed-softmax and P-packing code is flash_fwd_kernel's, and the
// second product O^T += V^T . P^T stays on v_mfma_f32_32x32x16_bf16 with the same V^T pre-pass and image.
// The factor 2^(eq + ek) is NOT put in the instruction's e8m0 scale operands: it is folded with scale * log2(e) into one
// fp32 constant per head, applied inside the exp2 argument as an FMA that replaces the subtraction of the running maximum
// (no extra instruction; the maximum itself is taken on the raw sums, the constant being positive).  The softmax scale
// cannot be multiplied into Q before quantisation as the bf16 kernel does: that would change the codes.

#include "flash_common.hip.h"

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
    auto Vs = [&](int buf) -> char* { return fl8_smem + 2 * FL8_K_BYTES + buf * FL8_V_BYTES; };

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, ql = lane & 31, h = lane >> 5;
    // workgroup id -> (kv head, query head in its group, query tile, KV run), heavy tiles first: flash_fwd_kernel's order
    const int rep = hq / hkv, nqt = (q_len + FL_BQ - 1) / FL_BQ;
    const int id = blockIdx.x;
    const int kvh = id % hkv, rest = id / hkv;
    const int head = kvh * rep + rest % rep;
    const int rest2 = rest / rep;
    int order = rest2;
    const int nord = nqt * sp.nsplit;
    if (sp.nsplit > 1 && order >= nord / 2) order = nord / 2 + (nord - 1 - order);
    const int split = order % sp.nsplit;
    const int qt = nqt - 1 - order / sp.nsplit;
    const int qw0 = qt * FL_BQ + wid * 32;          // first query row of this wave
    const int causal_off = kv_len - q_len;
    const uint8_t* kh = k8 + (size_t)kvh * kv_len * D;
    const T* vh = vt + (size_t)kvh * D * kv_pad;
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

    const int q_last = min(qt * FL_BQ + FL_BQ - 1, q_len - 1);
    const int kv_end = min(kv_len, causal_off + q_last + 1);
    const int nt_all = (kv_end + FL_BKV - 1) / FL_BKV;
    // this workgroup's run of KV tiles [t0, t1)
    const int t0 = (int)((long long)nt_all * split / sp.nsplit), t1 = (int)((long long)nt_all * (split + 1) / sp.nsplit);

    // staging in named registers (see flash_fwd_kernel): K chunk i of this thread is row kr + 32 i, 16-byte chunk kc - a whole
    // tile is 8 KiB of contiguous codes, chunk index = tid + 256 i; V^T chunk i is row vd + 32 i, 16-byte chunk vc
    uint4 rk0, rk1, rv0, rv1, rv2, rv3;
    const int kr = tid >> 3, kc = tid & 7;
    const int vd = tid >> 3, vc = tid & 7;
    const uint32_t vo0 = (uint32_t)(vd * kv_pad + vc * 8), vo_step = (uint32_t)(32 * kv_pad);
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
    auto load_v = [&](int t) {
        const T* vtile = vh + t * FL_BKV;
        rv0 = *reinterpret_cast<const uint4*>(vtile + vo0);
        rv1 = *reinterpret_cast<const uint4*>(vtile + vo0 + vo_step);
        rv2 = *reinterpret_cast<const uint4*>(vtile + vo0 + 2 * vo_step);
        rv3 = *reinterpret_cast<const uint4*>(vtile + vo0 + 3 * vo_step);
    };
    auto put_v = [&](char* base, int d, const uint4& x) {
        *reinterpret_cast<uint2*>(base + fl_v_off(d, 2 * vc)) = make_uint2(x.x, x.y);
        *reinterpret_cast<uint2*>(base + fl_v_off(d, 2 * vc + 1)) = make_uint2(x.z, x.w);
    };
    auto store_k = [&](int buf) {
        char* kb = Ks(buf);
        *reinterpret_cast<uint4*>(kb + fl8_k_off(kr, kc)) = rk0;
        *reinterpret_cast<uint4*>(kb + fl8_k_off(kr + 32, kc)) = rk1;
    };
    auto store_v = [&](int buf) {
        char* vb = Vs(buf);
        put_v(vb, vd, rv0);
        put_v(vb, vd + 32, rv1);
        put_v(vb, vd + 64, rv2);
        put_v(vb, vd + 96, rv3);
    };
    auto k_frag = [&](int buf, int row, int s) -> i32x8_f8 {
        const uint4 lo = *reinterpret_cast<const uint4*>(Ks(buf) + fl8_k_off(row, 4 * s + 2 * h));
        const uint4 hi = *reinterpret_cast<const uint4*>(Ks(buf) + fl8_k_off(row, 4 * s + 2 * h + 1));
        return i32x8_f8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
    };
    // S^T = K . Q^T of one tile (raw fp8 sums): two 32-kv sub-tiles (rows = positions, column = this lane's query), two
    // 64-d steps each; cbsz = blgp = 0 selects e4m3 for both operands, scale operands 0 = the instruction's unscaled form
    auto qk = [&](int buf, f32x16_fl& s0, f32x16_fl& s1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { s0[r] = 0.f; s1[r] = 0.f; }
        const i32x8_f8 a00 = k_frag(buf, ql, 0), a10 = k_frag(buf, 32 + ql, 0);
        const i32x8_f8 a01 = k_frag(buf, ql, 1), a11 = k_frag(buf, 32 + ql, 1);
        s0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a00, qf0, s0, 0, 0, 0, 0, 0, 0);
        s1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a10, qf0, s1, 0, 0, 0, 0, 0, 0);
        s0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a01, qf1, s0, 0, 0, 0, 0, 0, 0);
        s1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a11, qf1, s1, 0, 0, 0, 0, 0, 0);
    };
    // tiles entirely above this wave's diagonal contribute nothing (wave-uniform)
    auto live = [&](int t) -> bool { return t < t1 && t * FL_BKV <= causal_off + qw0 + 31; };

    f32x16_fl sc0, sc1;
    if (t0 < t1) {
        load_k(t0);
        load_v(t0);
        store_k(t0 & 1);
        store_v(t0 & 1);
    }
    // retire the Q loads here, not behind the first tile prefetch (see flash_fwd_kernel)
#pragma unroll
    for (int j = 0; j < 8; ++j) asm volatile("" ::"v"(qf0[j]), "v"(qf1[j]));
    __syncthreads();
    typedef uint32_t fl_u32x2 __attribute__((ext_vector_type(2)));
    typedef __attribute__((address_space(3))) const volatile fl_u32x2* fl_lds_cv64;
    for (int t = t0; t < t1; ++t) {
        const int buf = t & 1, kv0 = t * FL_BKV;
        if (t + 1 < t1) { load_k(t + 1); load_v(t + 1); }
        const bool cur = live(t);
        if (cur) qk(buf, sc0, sc1);
        if (cur) {
            // ---- mask, online softmax (this lane: query qw0 + ql, kv rows (r&3) + 8(r>>2) + 4h of each sub-tile) ----
            const bool need_mask = kv0 + FL_BKV - 1 > causal_off + qw0 || kv0 + FL_BKV > kv_len;   // wave-uniform
            const int lim = min(causal_off + qw0 + ql, kv_len - 1) - kv0 - 4 * h;                  // local kv row <= lim is visible
            float mx = -INFINITY;
            if (need_mask) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kvl = (r & 3) + 8 * (r >> 2);
                    sc0[r] = kvl <= lim ? sc0[r] : -INFINITY;
                    sc1[r] = 32 + kvl <= lim ? sc1[r] : -INFINITY;
                }
            }
#pragma unroll
            for (int r = 0; r < 16; r += 2) mx = fmaxf(fmaxf(fmaxf(sc0[r], sc1[r]), fmaxf(sc0[r + 1], sc1[r + 1])), mx);
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64)) * cf;      // cf > 0: the maximum of the raw sums is the maximum of the scores
            // deferred rescale, as flash_fwd_kernel: the reference point moves only when the maximum grew by more than 6
            const float m_new = (mx > m_run + 6.0f || m_run == -INFINITY) ? fmaxf(m_run, mx) : m_run;
            const float m_use = m_new == -INFINITY ? 0.f : m_new;
            const bool moved = __builtin_amdgcn_ballot_w64(m_new != m_run) != 0;   // wave-uniform
            const float alpha = moved ? __builtin_amdgcn_exp2f(m_run - m_use) : 1.0f;
            float ls = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                sc0[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(sc0[r], cf, -m_use));
                sc1[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(sc1[r], cf, -m_use));
                ls += sc0[r] + sc1[r];
            }
            l_run = l_run * alpha + ls;
            m_run = m_new;
            if (moved) {
#pragma unroll
                for (int i = 0; i < DT; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[i][r] *= alpha;
            }
            // ---- O^T += V^T . P^T : 4 k-steps of 16 kv, flash_fwd_kernel's V^T reads (volatile 8-byte LDS reads) ----
            const char* vrow = Vs(buf) + ql * 128;
            const int vsw = (ql >> 1) & 15;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                uint4 pb;
                if (s < 2) {
                    pb = make_uint4(pack_bf16x2(sc0[8 * s + 0], sc0[8 * s + 1]), pack_bf16x2(sc0[8 * s + 2], sc0[8 * s + 3]),
                                    pack_bf16x2(sc0[8 * s + 4], sc0[8 * s + 5]), pack_bf16x2(sc0[8 * s + 6], sc0[8 * s + 7]));
                } else {
                    pb = make_uint4(pack_bf16x2(sc1[8 * (s - 2) + 0], sc1[8 * (s - 2) + 1]), pack_bf16x2(sc1[8 * (s - 2) + 2], sc1[8 * (s - 2) + 3]),
                                    pack_bf16x2(sc1[8 * (s - 2) + 4], sc1[8 * (s - 2) + 5]), pack_bf16x2(sc1[8 * (s - 2) + 6], sc1[8 * (s - 2) + 7]));
                }
#pragma unroll
                for (int i = 0; i < DT; ++i) {
                    const fl_u32x2 lo = *(fl_lds_cv64)(vrow + (((4 * s + h) ^ vsw) << 3) + i * 4096);
                    const fl_u32x2 hi = *(fl_lds_cv64)(vrow + (((4 * s + 2 + h) ^ vsw) << 3) + i * 4096);
                    o[i] = mfma32<T>(make_uint4(lo.x, lo.y, hi.x, hi.y), pb, o[i]);
                }
            }
        }
        if (t + 1 < t1) { store_k(buf ^ 1); store_v(buf ^ 1); }
        __syncthreads();
    }

    // ---- normalise and store: lane = query row, registers 4g..4g+3 of tile i are d = 32i + 8g + 4h .. +3 ----
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
    const int qrow = qw0 + ql;
    if (qrow < q_len) {
        T* orow = sp.nsplit > 1 ? reinterpret_cast<T*>(sp.o) + (((size_t)split * q_len + qrow) * hq + head) * D
                                : out + (size_t)head * sd.oh + (size_t)qrow * sd.os;
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                uint2 w;
                w.x = pack_bf16x2(o[i][4 * g] * inv, o[i][4 * g + 1] * inv);
                w.y = pack_bf16x2(o[i][4 * g + 2] * inv, o[i][4 * g + 3] * inv);
                *reinterpret_cast<uint2*>(orow + i * 32 + 8 * g + 4 * h) = w;
            }
        if (sp.nsplit > 1 && h == 0) {
            float* ml = sp.ml + (((size_t)split * hq + head) * q_len + qrow) * 2;
            ml[0] = m_run;
            ml[1] = l_tot;
        }
    }
}

static size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

static pgk_status flash_fp8_launch(const bf16* q, const bf16* k, const bf16* v, bf16* out, int hq, int hkv, int q_len, int kv_len, float scale,
                                   const FlashStrides& sd, hipStream_t st) {
    constexpr int D = 128;
    const int kv_pad = ceil_div(kv_len, 64) * 64;
    const int nqt = ceil_div(q_len, FL_BQ);
    const int nsplit = flash_nsplit(nqt, hq, kv_len, device_cu_count());      // the bf16 kernel's choice: same occupancy, same tile walk
    const size_t vt_bytes = up256((size_t)hkv * D * kv_pad * sizeof(bf16));
    const size_t po_bytes = nsplit > 1 ? up256((size_t)nsplit * q_len * hq * D * sizeof(bf16)) : 0;
    const size_t ml_bytes = nsplit > 1 ? up256((size_t)nsplit * hq * q_len * 2 * sizeof(float)) : 0;
    const size_t q8_bytes = up256((size_t)hq * q_len * D), k8_bytes = up256((size_t)hkv * kv_len * D);
    const size_t am_bytes = up256((size_t)(hq + hkv) * sizeof(uint32_t)), sb_bytes = up256((size_t)(hq + hkv));
    void* ws = nullptr;
    if (pgk_status r = pgk_malloc(&ws, vt_bytes + po_bytes + ml_bytes + q8_bytes + k8_bytes + am_bytes + sb_bytes)) return r;
    char* p = (char*)ws;
    bf16* vt = (bf16*)p; p += vt_bytes;
    FlashSplit sp{nsplit, nullptr, nullptr, nullptr, nullptr};
    if (nsplit > 1) {
        sp.o = p; p += po_bytes;
        sp.ml = (float*)p; p += ml_bytes;
    }
    uint8_t* q8 = (uint8_t*)p; p += q8_bytes;
    uint8_t* k8 = (uint8_t*)p; p += k8_bytes;
    uint32_t* amax = (uint32_t*)p; p += am_bytes;
    uint8_t* sb = (uint8_t*)p;
    hipError_t e = hipMemsetAsync(amax, 0, (size_t)(hq + hkv) * sizeof(uint32_t), st);
    pgk_status r = PGK_OK;
    if (e == hipSuccess) {
        const Fp8HeadSrc qs{q, q8, sb, amax, hq, q_len, sd.qh, sd.qs}, ks{k, k8, sb + hq, amax + hq, hkv, kv_len, sd.kh, sd.ks};
        r = fp8_quantize_heads(qs, ks, st);
    }
    if (e == hipSuccess && r == PGK_OK) {
        transpose_v_kernel<bf16, D><<<dim3(kv_pad / 64, hkv), 256, 0, st>>>(v, vt, kv_len, kv_pad, sd.kh, sd.ks);
        flash_fwd_fp8_kernel<<<nqt * hq * nsplit, FL_THREADS, FL8_LDS, st>>>(q8, k8, sb, sb + hq, vt, out, hq, hkv, q_len, kv_len, kv_pad,
                                                                            scale * 1.4426950408889634f, sd, sp);
        e = hipGetLastError();
        if (e == hipSuccess && nsplit > 1) {
            const size_t work = (size_t)q_len * hq * (D / 8);
            flash_merge_kernel<bf16, D><<<(unsigned)((work + 255) / 256), 256, 0, st>>>(sp.ml, (const bf16*)sp.o, out, hq, q_len, nsplit, sd.oh, sd.os);
            e = hipGetLastError();
        }
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
