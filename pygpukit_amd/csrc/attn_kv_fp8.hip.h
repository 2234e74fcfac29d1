// Split-KV decode of ONE query row over an FP8 (OCP e4m3) KV cache [Hkv][max_seq][D] in uint8, with one fp32 scale per KV head for K
// and one for V (value = e4m3(code) * scale).  ops_kv_fp8.hip is the only user.
//
// The chunking, the partial record [m, l, o[D]] and the second phase are attn_core.hip.h's (decode_chunk_len, decode_phase2_kernel);
// the walk is its own, because a row is D BYTES here:
//   * D/16 lanes cover a row with one 16-byte load each (8 lanes at D = 128, 4 at D = 64): a wave instruction still fetches 1 KiB
//     contiguous, but 8 / 16 positions of it, and a lane owns 16 head dims.  4 waves step 32 / 64 positions (KV8_STEP).
//   * the scales cost nothing in the walk: k_scale joins the softmax scale in the query premultiply, v_scale multiplies the
//     un-normalised o once, where the workgroup writes its partial record.
//   * what remains is the conversion, which is exact (e4m3 is a subset of bf16): v_cvt_scalef32_pk_bf16_fp8 with scale 1 turns two
//     codes into one dword of bf16, and the dot products run on v_dot2_f32_bf16 as kv_consume's do.  For V the codes of two rows are
//     interleaved by v_perm_b32 BEFORE the conversion (bytes, so 2 perms per 4 dims of a row pair - half of what interleaving the
//     bf16 words costs), and the converted dword (v_u[j], v_u'[j]) meets the packed probabilities (p_u, p_u').
//   * trips of U position-groups: all 2 U loads are issued before the first is consumed, one running-max update per trip.  Load
//     addresses are clamped to the chunk's last LIVE row, so no byte at or beyond ctx is ever fetched: a cache is uninitialised
//     memory there, NaN codes included, and 0 * NaN is NaN.  Scores of masked positions are SELECTED to -inf, never multiplied.
//   * the 8 / 16 lane-groups of a wave are folded to 4 (one per 16-lane row) with DPP row rotations before LDS, so the merge is
//     attn_core's 16 slots: 4 * 16 * G * (D + 2) floats = 33 KiB at D = 128, G = 4 (one slot per lane-group would need 66 KiB).
#pragma once

#include "attn_core.hip.h"

namespace pgk {

template <int D> constexpr int kv8_step() { return 4 * (64 / (D / 16)); }   // positions per step of 4 waves: decode_chunk_len's gran

// two e4m3 codes (bytes 0, 1 or 2, 3 of w) -> one dword of bf16, exact
template <bool HI>
__device__ __forceinline__ uint32_t kv8_cvt(uint32_t w) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, HI));
}

// The cache writers' quantiser (kv8_write_kernel, paged_kv8_write_kernel): 16 elements at src -> 16 codes, rne_e4m3(clamp(x / sc,
// +-448)) with x widened to fp32 and a correctly rounded division.  The clamp runs in fp32 BEFORE the conversion (fmaxf / fminf
// also turn a NaN into a finite bound): 0x7F / 0xFF are never written; -0 stays -0 through both and converts to 0x80.
template <class T>
__device__ __forceinline__ uint4 kv8_quantise16(const T* src, float sc) {
    constexpr float E4M3_MAX = 448.f;
    float f[2][8];
    KVLoad<T>::load8(src, f[0]);
    KVLoad<T>::load8(src + 8, f[1]);
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float c[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = fminf(fmaxf(__fdiv_rn(f[i >> 1][(4 * i + j) & 7], sc), -E4M3_MAX), E4M3_MAX);
        w[i] = pack_fp8x4(c[0], c[1], c[2], c[3]);
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

constexpr int DPP_ROR4 = 0x124;   // rotate by 4 within each 16

// all-reduce over the LPR = 8 / 4 lanes of a row
template <int LPR> __device__ __forceinline__ float kv8_row_sum(float v) {
    v += dpp_f<DPP_XOR1>(v); v += dpp_f<DPP_XOR2>(v);
    if constexpr (LPR == 8) v += dpp_f<DPP_HALF_MIRROR>(v);
    return v;
}
// sum over the 2 / 4 lane-groups that share a 16-lane DPP row (lanes with equal lane % LPR); every lane gets the total
template <int LPR> __device__ __forceinline__ float kv8_fold16(float v) {
    v += dpp_f<DPP_ROR8>(v);
    if constexpr (LPR == 4) v += dpp_f<DPP_ROR4>(v);
    return v;
}

template <int G>
struct KV8State {
    float m[G], l[G], o[G][16];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            m[g] = -INFINITY; l[g] = 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j) o[g][j] = 0.f;
        }
    }
};

template <int U> struct KV8Batch { uint4 k[U], v[U]; };

// K rows first, then V rows (vector memory returns in issue order: the scores run while V is still arriving).  clamp_max: last live row
template <int D, int U>
__device__ __forceinline__ void kv8_issue(KV8Batch<U>& kb, const uint8_t* kbase, const uint8_t* vbase, int p0, int clamp_max, int lane) {
    constexpr int LPR = D / 16, STEP = kv8_step<D>();
    const int grp = lane / LPR, sub = lane % LPR;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int pc = min(p0 + u * STEP + grp, clamp_max);
        kb.k[u] = *reinterpret_cast<const uint4*>(kbase + (size_t)pc * D + sub * 16);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int pc = min(p0 + u * STEP + grp, clamp_max);
        kb.v[u] = *reinterpret_cast<const uint4*>(vbase + (size_t)pc * D + sub * 16);
    }
}

// qb[g][i]: bf16 pair (dims 2 i, 2 i + 1 of this lane's 16) of query head g, premultiplied by scale * k_scale.
// VALU instructions per position and lane-group (ISA count in DESIGN.md 4.4): 8 conversions + G * (8 dot2 + row sum) for the
// score, 4 perms + 8 conversions + G * 8 dot2 for P.V, and the softmax's handful per head.
template <int D, int G, int U>
__device__ __forceinline__ void kv8_consume(const KV8Batch<U>& kb, int p0, int c1, const uint32_t (&qb)[G][8], int lane, KV8State<G>& st) {
    constexpr int LPR = D / 16, STEP = kv8_step<D>();
    static_assert(U % 2 == 0, "positions are consumed in pairs");
    const int grp = lane / LPR;
    float s[U][G];
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int g = 0; g < G; ++g) s[u][g] = -INFINITY;
        if (p0 + u * STEP < c1) {                               // wave-uniform: some lane-group of this wave has a live position
            const bool valid = p0 + u * STEP + grp < c1;
            const uint32_t w[4] = {kb.k[u].x, kb.k[u].y, kb.k[u].z, kb.k[u].w};
            uint32_t kw[8];
#pragma unroll
            for (int i = 0; i < 4; ++i) { kw[2 * i] = kv8_cvt<false>(w[i]); kw[2 * i + 1] = kv8_cvt<true>(w[i]); }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                float d = 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) d = attn_dot2(kw[i], qb[g][i], d);
                d = kv8_row_sum<LPR>(d);
                s[u][g] = valid ? d : -INFINITY;                // a select: the clamped row's score must not count twice
            }
        }
    }
    float mx[G], alpha[G], lsum[G];
    bool any[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        mx[g] = st.m[g];
#pragma unroll
        for (int u = 0; u < U; ++u) mx[g] = fmaxf(mx[g], s[u][g]);
        any[g] = mx[g] != -INFINITY;                            // nothing live yet for this lane-group: leave the state alone
        alpha[g] = any[g] ? __expf(st.m[g] - mx[g]) : 1.f;
        lsum[g] = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) st.o[g][j] *= alpha[g];
    }
#pragma unroll
    for (int u = 0; u < U; u += 2) {
        if (p0 + u * STEP < c1) {                               // wave-uniform
            // codes of rows u (a) and u + 1 (b), dims 4 i .. 4 i + 3 per word -> {a[j], b[j], a[j+1], b[j+1]} -> two bf16 pairs
            const uint32_t a[4] = {kb.v[u].x, kb.v[u].y, kb.v[u].z, kb.v[u].w};
            const uint32_t b[4] = {kb.v[u + 1].x, kb.v[u + 1].y, kb.v[u + 1].z, kb.v[u + 1].w};
            uint32_t vw[16];                                    // vw[j] = (v_u[j], v_u'[j]) as bf16
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t lo = __builtin_amdgcn_perm(b[i], a[i], 0x05010400u);   // {a.b0, b.b0, a.b1, b.b1}
                const uint32_t hi = __builtin_amdgcn_perm(b[i], a[i], 0x07030602u);   // {a.b2, b.b2, a.b3, b.b3}
                vw[4 * i] = kv8_cvt<false>(lo); vw[4 * i + 1] = kv8_cvt<true>(lo);
                vw[4 * i + 2] = kv8_cvt<false>(hi); vw[4 * i + 3] = kv8_cvt<true>(hi);
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const float pa = any[g] ? __expf(s[u][g] - mx[g]) : 0.f;        // exp(-inf) = 0 for masked positions
                const float pb = any[g] ? __expf(s[u + 1][g] - mx[g]) : 0.f;
                const uint32_t pk = pack_bf16x2(pa, pb);
                // the denominator sums the ROUNDED probabilities, the ones the numerator uses
                lsum[g] += __uint_as_float(pk << 16) + __uint_as_float(pk & 0xFFFF0000u);
#pragma unroll
                for (int j = 0; j < 16; ++j) st.o[g][j] = attn_dot2(vw[j], pk, st.o[g][j]);
            }
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (any[g]) {
            st.l[g] = st.l[g] * alpha[g] + lsum[g];
            st.m[g] = mx[g];
        }
    }
}

// Fold the lane-groups of each 16-lane row, merge the 16 rows of the workgroup through LDS (>= 16 * G * (D + 2) floats) and write the
// chunk's G partial records, o multiplied by v_scale.  `part`: record of head g = 0; consecutive heads are head_stride floats apart.
template <int D, int G>
__device__ __forceinline__ void kv8_block_merge(KV8State<G>& st, float* lds, float* part, size_t head_stride, float v_scale, int lane,
                                                int wid) {
    constexpr int LPR = D / 16, NS = 16, RS = D + 2;
    const int sub = lane % LPR, slot = wid * 4 + (lane >> 4);
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const float mr = group16_max(st.m[g]);
        const float w = st.m[g] == -INFINITY ? 0.f : __expf(st.m[g] - mr);
        const float l = kv8_fold16<LPR>(st.l[g] * w);
        float* rec = lds + ((size_t)slot * G + g) * RS;
        if ((lane & 15) == 0) { rec[0] = mr; rec[1] = l; }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float o = kv8_fold16<LPR>(st.o[g][j] * w);
            if ((lane & 15) < LPR) rec[2 + sub * 16 + j] = o;
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < G * D; e += blockDim.x) {
        const int g = e / D, d = e % D;
        float mx = -INFINITY;
#pragma unroll
        for (int s = 0; s < NS; ++s) mx = fmaxf(mx, lds[((size_t)s * G + g) * RS]);
        float l = 0.f, o = 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const float* rec = lds + ((size_t)s * G + g) * RS;
            const float w = (rec[0] == -INFINITY) ? 0.f : __expf(rec[0] - mx);
            l = fmaf(rec[1], w, l);
            o = fmaf(rec[2 + d], w, o);
        }
        float* outrec = part + (size_t)g * head_stride;
        outrec[2 + d] = o * v_scale;
        if (d == 0) { outrec[0] = mx; outrec[1] = l; }
    }
}

// Phase 1: workgroup (chunk, group of G consecutive query heads of one kv head) -> G partial records.  ctx = ctx_buf[0] or host_ctx,
// clamped to [0, max_seq] (pgk_sdpa_fixed_cache's clamp).
template <class T, int D, int G>
__global__ __launch_bounds__(256) void kv8_decode_phase1_kernel(const T* q, const uint8_t* kc, const uint8_t* vc, const float* k_scale,
                                                                const float* v_scale, float* ws, int hq, int hkv, int max_seq, int nsplit,
                                                                float scale, int host_ctx, const int32_t* ctx_buf) {
    constexpr int LPR = D / 16, PPW = 64 / LPR, STEP = kv8_step<D>(), RS = D + 2, U = 4;
    __shared__ float lds[16 * G * RS];
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), sub = lane % LPR;
    const int ctx = max(min(ctx_buf ? ctx_buf[0] : host_ctx, max_seq), 0);
    const int h0 = blockIdx.y * G, kv_head = h0 / (hq / hkv);
    const int chunk = decode_chunk_len(ctx, nsplit, STEP);
    const int c0 = min((int)blockIdx.x * chunk, ctx), c1 = min(c0 + chunk, ctx);
    const float qmul = scale * k_scale[kv_head];
    uint32_t qb[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        float f[2][8];
        KVLoad<T>::load8(q + (size_t)(h0 + g) * D + sub * 16, f[0]);
        KVLoad<T>::load8(q + (size_t)(h0 + g) * D + sub * 16 + 8, f[1]);
#pragma unroll
        for (int i = 0; i < 8; ++i) qb[g][i] = pack_bf16x2(f[i >> 2][(2 * i) & 7] * qmul, f[i >> 2][(2 * i + 1) & 7] * qmul);
    }
    KV8State<G> st;
    st.init();
    const uint8_t* kbase = kc + (size_t)kv_head * max_seq * D;
    const uint8_t* vbase = vc + (size_t)kv_head * max_seq * D;
    for (int b0 = c0; b0 < c1; b0 += U * STEP) {                 // workgroup-uniform trip count; c1 - 1 >= 0 inside
        const int p0 = b0 + wid * PPW;
        KV8Batch<U> kb;
        kv8_issue<D, U>(kb, kbase, vbase, p0, c1 - 1, lane);
        kv8_consume<D, G, U>(kb, p0, c1, qb, lane, st);
    }
    kv8_block_merge<D, G>(st, lds, ws + ((size_t)h0 * nsplit + blockIdx.x) * RS, (size_t)nsplit * RS, v_scale[kv_head], lane, wid);
}

}  // namespace pgk
