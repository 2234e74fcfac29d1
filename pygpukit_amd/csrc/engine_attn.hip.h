// Decode attention kernels (split-KV, whole-context, fused / merged o_proj) and their launcher.
#pragma once

#include "attn_core.hip.h"
#include "attn_tail_plan.h"
#include "engine_state.hip.h"
#include "lds_dma.hip.h"

namespace pgk {

// --------------------------------------------------------------------------------------------
// Decode attention.  Shared front end: QK-norm + RoPE of the new token's q/k, bf16 rounding of k/v.
// --------------------------------------------------------------------------------------------
struct AttnArgs {
    const float* qkv;     // [B][(Hq+2Hkv)*D] fp32, pre-norm
    int qkv_ld;
    const bf16 *q_gamma, *k_gamma;
    float eps;
    const float *rope_cos, *rope_sin;   // [B][D/2]: the table rows of each sequence's CURRENT position
    bf16 *kcache, *vcache;              // this layer: [B][Hkv][max_seq][D]
    const int32_t* positions;
    int hq, hkv, max_seq;
    int span;             // split path: the positions [0, span) are what the slices cover (<= max_seq: the step's context tier, Engine::step_span)
    float scale;
    // split path
    float* part;          // [B][Hq][nsplit][D+2]
    int nsplit;
    float* attn_direct;   // whole-context variant (nsplit == 1): normalised output [B][Hq][D], no merge launch
    // fused o_proj path
    const bf16* w_o;      // [H][Hq*D] (fp8 codes on the merged o_proj path with fp8 weights)
    const bf16* w_o_scale; // fp8 W_o: [H/128][Hq*D/128] block scales
    int H, rows_per_block;
    float* opart;         // [B][Hkv][H]
    bf16* attn_direct16;  // whole-context variant: bf16 output instead of attn_direct (batched MFMA o_proj reads it)
    // GQA groups other than the instantiated 1 / 2 / 4 query heads per kv head run as several launches over head chunks:
    // this launch serves query heads kvh * g_total + g_off + [0, G) of every kv head (ordinary launch: g_total = G, g_off = 0)
    int g_total, g_off;
};

template <int D, int G>
struct NewToken {
    float qf[G][8], kn[8], vn[8];   // q (pre-scaled) and k, v of the new token, all as the bf16-rounded values every consumer sees
    uint4 qb[G], kbits, vbits;      // the same as packed bf16
};

// The new token's q/k/v, in two steps so that a kernel can put other loads between them: (1) every load - the fp32 q/k/v
// row slices of this lane, the QK-norm gammas, the RoPE row - issued back to back, nothing waited for; (2) pure ALU.
// Vector memory returns in issue order, so whatever is loaded FIRST is usable first: the fused kernel issues these small
// L2-resident loads ahead of its K/V and W_o streams and runs step (2) while those are still in flight.
template <int G>
struct NewTokenRaw {
    float4 lo[G + 2], hi[G + 2];   // q heads, k, v: this lane's 8 dims
    uint4 gq, gk;                  // 8 bf16 gammas each
    float4 cs[2], sn[2];           // RoPE row slice
};

template <int D, int G>
__device__ __forceinline__ void new_token_load(const AttnArgs& a, int b, int kvh, int lane, NewTokenRaw<G>& r) {
    constexpr int LPR = D / 8, HALF = D / 2;
    const int sub = lane % LPR;
    const float* row = a.qkv + (size_t)b * a.qkv_ld;
#pragma unroll
    for (int g = 0; g < G + 2; ++g) {
        const unsigned eoff = (g < G) ? (unsigned)(kvh * a.g_total + a.g_off + g) * D : (g == G ? (unsigned)(a.hq + kvh) * D : (unsigned)(a.hq + a.hkv + kvh) * D);
        r.lo[g] = *reinterpret_cast<const float4*>(row + eoff + sub * 8);
        r.hi[g] = *reinterpret_cast<const float4*>(row + eoff + sub * 8 + 4);
    }
    r.gq = r.gk = make_uint4(0, 0, 0, 0);
    if (a.q_gamma != nullptr) {
        r.gq = *reinterpret_cast<const uint4*>(a.q_gamma + sub * 8);
        r.gk = *reinterpret_cast<const uint4*>(a.k_gamma + sub * 8);
    }
    const int dd = (sub * 8) % HALF;                    // the lane's 8 dims stay inside one half (8 | HALF)
    const float* cs = a.rope_cos + (size_t)b * HALF + dd;   // address independent of the position: no extra round trip
    const float* sn = a.rope_sin + (size_t)b * HALF + dd;
    r.cs[0] = *reinterpret_cast<const float4*>(cs); r.cs[1] = *reinterpret_cast<const float4*>(cs + 4);
    r.sn[0] = *reinterpret_cast<const float4*>(sn); r.sn[1] = *reinterpret_cast<const float4*>(sn + 4);
}

template <int D, int G>
__device__ __forceinline__ void new_token_finish(const AttnArgs& a, int lane, const NewTokenRaw<G>& r, NewToken<D, G>& t) {
    constexpr int LPR = D / 8;
    const int sub = lane % LPR;
    float raw[G + 2][8], gq[8], gk[8];
#pragma unroll
    for (int g = 0; g < G + 2; ++g) {
        raw[g][0] = r.lo[g].x; raw[g][1] = r.lo[g].y; raw[g][2] = r.lo[g].z; raw[g][3] = r.lo[g].w;
        raw[g][4] = r.hi[g].x; raw[g][5] = r.hi[g].y; raw[g][6] = r.hi[g].z; raw[g][7] = r.hi[g].w;
    }
    const bool has_norm = a.q_gamma != nullptr;
    if (has_norm) {
        WTraits<bf16>::decode(r.gq, gq);
        WTraits<bf16>::decode(r.gk, gk);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) gq[j] = gk[j] = 1.f;
    }
    const float csv[8] = {r.cs[0].x, r.cs[0].y, r.cs[0].z, r.cs[0].w, r.cs[1].x, r.cs[1].y, r.cs[1].z, r.cs[1].w};
    const float snv[8] = {r.sn[0].x, r.sn[0].y, r.sn[0].z, r.sn[0].w, r.sn[1].x, r.sn[1].y, r.sn[1].z, r.sn[1].w};
    // norm + rope of one head vector; this lane holds dims sub*8..+8, the rotate-half partner dims live
    // LPR/2 lanes away.
    auto norm_rope = [&](const float (&xin)[8], const float (&gamma)[8], float (&o)[8]) {
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = xin[j];
        if (has_norm) {
            float ss = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) ss = fmaf(x[j], x[j], ss);
            ss = group_sum<LPR>(ss);
            const float inv = 1.0f / sqrtf(ss / D + a.eps);
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = x[j] * inv * gamma[j];
        }
        const bool lo = sub < LPR / 2;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float other = xor_half<LPR>(x[j]);
            o[j] = lo ? (x[j] * csv[j] - other * snv[j]) : (x[j] * csv[j] + other * snv[j]);
        }
    };
#pragma unroll
    for (int g = 0; g < G; ++g) {
        norm_rope(raw[g], gq, t.qf[g]);
#pragma unroll
        for (int j = 0; j < 8; ++j) t.qf[g][j] *= a.scale;
        Vec<bf16> qv;                   // q is bf16 from here on (the model's dtype): scores run on the packed bf16 dot
        qv.from_float(t.qf[g]);
        qv.to_float(t.qf[g]);
        t.qb[g] = qv.raw;
    }
    norm_rope(raw[G], gk, t.kn);
#pragma unroll
    for (int j = 0; j < 8; ++j) t.vn[j] = raw[G + 1][j];
    // the cache holds bf16: this step uses the rounded values too (identical to reading them back)
    Vec<bf16> kb, vb;
    kb.from_float(t.kn);
    vb.from_float(t.vn);
    kb.to_float(t.kn);
    vb.to_float(t.vn);
    t.kbits = kb.raw;
    t.vbits = vb.raw;
}

template <int D, int G>
__device__ __forceinline__ void prepare_new_token(const AttnArgs& a, int b, int kvh, int pos, int lane, NewToken<D, G>& t) {
    NewTokenRaw<G> r;
    new_token_load<D, G>(a, b, kvh, lane, r);
    new_token_finish<D, G>(a, lane, r, t);
}

template <int D, int G>
__device__ __forceinline__ void fold_new_token(const NewToken<D, G>& t, DecodeState<G>& st) {
    constexpr int LPR = D / 8;
    float s[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        float dsum = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) dsum = fmaf(t.qf[g][j], t.kn[j], dsum);
        dsum = group_sum<LPR>(dsum);
        s[g] = dsum;
    }
    st.update(s, t.vn);
}

// split path: grid (nsplit, Hkv, batch)
template <int D, int G, bool DIRECT>
__global__ __launch_bounds__(256) void attn_decode_kernel(unsigned long long* tl, AttnArgs a) {
    const TLStamp tls(tl);
    constexpr int LPR = D / 8, PPW = 64 / LPR, RS = D + 2;
    __shared__ __attribute__((aligned(16))) float lds[4 * PPW * G * RS];
    __shared__ float attn_out[DIRECT ? G * D : 1];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, sub = lane % LPR;
    const int kvh = blockIdx.y, b = blockIdx.z;
    const size_t head_off = (((size_t)b * a.hkv + kvh) * a.max_seq) * D;
    if constexpr (DIRECT) {
        // One workgroup owns the whole (short) context.  As in attn_oproj_kernel, the first U0 position-groups per wave
        // are loaded from clamped addresses BEFORE the position is known, so the K/V bytes, the q/k/v row and the
        // position share one memory round trip (the split path below learns the position first, then walks:
        // two dependent trips - 9.2 us against 6.x for 8 sequences).
        // The position-independent part is the first 128 rows; rows 128-191 are requested as soon as the position is there
        // (a scalar load that overtakes the vector loads in flight), clamped to the LAST CACHED ROW instead of the cache's
        // last row: with 64 sequences at context ~150 every workgroup used to pull 192 rows whatever the context - 50 MB per
        // layer for 39 MB of live K/V, and this kernel is bandwidth-bound at that batch (3.2 TB/s of live bytes).
        constexpr int U0 = 8, UB = 4;
        NewTokenRaw<G> raw;                 // issue order = arrival order: the few L2-resident q/k/v bytes first, then the K/V rows
        new_token_load<D, G>(a, b, kvh, lane, raw);
        __builtin_amdgcn_sched_barrier(0);
        KVBatch<U0> kb0;
        kv_issue<D, U0, 4>(kb0, a.kcache + head_off, a.vcache + head_off, wid * PPW, a.max_seq - 1, lane);
        __builtin_amdgcn_sched_barrier(0);
        const int pos = load_uniform_i32(a.positions + b);   // scalar path (pgk_device.hip.h): not queued behind the vector loads in flight
        const int c1 = min(pos, a.max_seq);
        KVBatch<UB> kb1;
        kv_issue<D, UB, 4>(kb1, a.kcache + head_off, a.vcache + head_off, U0 * 4 * PPW + wid * PPW, max(c1 - 1, 0), lane);
        __builtin_amdgcn_sched_barrier(0);
        NewToken<D, G> t;
        new_token_finish<D, G>(a, lane, raw, t);
        if (pos < a.max_seq && wid == 0 && lane < LPR && a.g_off == 0) {
            *reinterpret_cast<uint4*>(a.kcache + head_off + (size_t)pos * D + sub * 8) = t.kbits;
            *reinterpret_cast<uint4*>(a.vcache + head_off + (size_t)pos * D + sub * 8) = t.vbits;
        }
        DecodeState<G> st;
        st.init();
        kv_consume<D, G, U0, 4>(kb0, wid * PPW, c1, t.qb, lane, st);
        kv_consume<D, G, UB, 4>(kb1, U0 * 4 * PPW + wid * PPW, c1, t.qb, lane, st);
        if (c1 > (U0 + UB) * 4 * PPW) decode_walk_trips<D, G>(a.kcache + head_off, a.vcache + head_off, (U0 + UB) * 4 * PPW, c1, t.qb, lane, wid, st);
        if (pos < a.max_seq && wid == 0 && lane < LPR) fold_new_token<D, G>(t, st);
        decode_block_merge_lds<D, G>(st, lds, attn_out, lane, wid);
        if (a.attn_direct16) {
            for (int e = threadIdx.x; e < G * D; e += 256) a.attn_direct16[((size_t)b * a.hq + (size_t)kvh * a.g_total + a.g_off) * D + e] = from_f<bf16>(attn_out[e]);
        } else {
            for (int e = threadIdx.x; e < G * D; e += 256) a.attn_direct[((size_t)b * a.hq + (size_t)kvh * a.g_total + a.g_off) * D + e] = attn_out[e];
        }
        tls.end();
        return;
    }
    // Slices are cut by ABSOLUTE position (slice s = cache rows [s * chunk, (s + 1) * chunk), chunk from the step's context tier a.span <= cache length):
    // no address depends on the context length, so the new token's q/k/v and the slice's first 128 K/V rows are requested
    // before the position is even known (clamped addresses; masked later).  Before, the walk started one scalar and one
    // vector round trip later (position -> slice bounds -> addresses).  Slices beyond the context write empty records.
    constexpr int U1 = 8;
    const int chunk = decode_chunk_len(a.span, a.nsplit, 4 * PPW);
    const int c0 = (int)blockIdx.x * chunk;
    NewTokenRaw<G> raw;
    new_token_load<D, G>(a, b, kvh, lane, raw);
    __builtin_amdgcn_sched_barrier(0);
    KVBatch<U1> kb0;
    kv_issue<D, U1, 4>(kb0, a.kcache + head_off, a.vcache + head_off, c0 + wid * PPW, a.max_seq - 1, lane);
    __builtin_amdgcn_sched_barrier(0);
    const int pos = load_uniform_i32(a.positions + b);   // scalar path (pgk_device.hip.h): not queued behind the vector loads in flight
    const int ctx = min(pos + 1, a.max_seq);
    tls.phase(0);
    NewToken<D, G> t;
    new_token_finish<D, G>(a, lane, raw, t);
    tls.phase(1);
    // the LAST slice runs to the end of the context wherever that is: the tier (a.span) comes from a host-side bound on the
    // position, and a caller that moved the device-resident positions past it behind the library's back must lose speed, not rows
    const bool last_slice = (int)blockIdx.x == a.nsplit - 1;
    const int c1 = last_slice ? ctx : min(c0 + chunk, ctx);
    const bool owns_new = (pos < a.max_seq) && (pos >= c0) && (last_slice || pos < c0 + chunk);
    if (owns_new && wid == 0 && lane < LPR && a.g_off == 0) {
        *reinterpret_cast<uint4*>(a.kcache + head_off + (size_t)pos * D + sub * 8) = t.kbits;
        *reinterpret_cast<uint4*>(a.vcache + head_off + (size_t)pos * D + sub * 8) = t.vbits;
    }
    DecodeState<G> st;
    st.init();
    const int cend = owns_new ? min(c1, pos) : c1;       // cached rows of this slice; the new token's row is folded from registers
    kv_consume<D, G, U1, 4>(kb0, c0 + wid * PPW, cend, t.qb, lane, st);
    if (cend > c0 + U1 * 4 * PPW)
        decode_walk_trips<D, G>(a.kcache + head_off, a.vcache + head_off, c0 + U1 * 4 * PPW, cend, t.qb, lane, wid, st);
    if (owns_new && wid == 0 && lane < LPR) fold_new_token<D, G>(t, st);
    tls.phase(2);
    if constexpr (DIRECT) {
        // this workgroup saw the whole context: normalise here and skip the merge launch
        decode_block_merge_lds<D, G>(st, lds, attn_out, lane, wid);
        for (int e = threadIdx.x; e < G * D; e += 256) a.attn_direct[((size_t)b * a.hq + (size_t)kvh * a.g_total + a.g_off) * D + e] = attn_out[e];
    } else {
        decode_block_merge<D, G>(st, lds, a.part + (((size_t)b * a.hq + (size_t)kvh * a.g_total + a.g_off) * a.nsplit + blockIdx.x) * RS,
                                 (size_t)a.nsplit * RS, lane, wid);
    }
    tls.end();
}

// split path, step 2: merge the nsplit (<= 64) chunk records of every head into the normalised attention
// vector attn[b][h*D + d] (fp32).  grid (Hq, batch), D threads (D = 64 or 128: whole waves).  Lane s of wave 0
// owns record s's (m, l): one load each, a wave max and a wave sum give the weights; then every thread sums its
// element over the records with independent loads.
template <int D>
__global__ void attn_merge_kernel(unsigned long long* tl, const float* part, float* attn, int hq, int nsplit) {
    const TLStamp tls(tl);
    __shared__ float w_s[64];
    __shared__ float inv_l;
    const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
    const float* recs = part + ((size_t)b * hq + h) * nsplit * (D + 2);
    if (threadIdx.x < 64) {
        const int s = threadIdx.x;
        const int sc = min(s, nsplit - 1);
        float m = recs[(size_t)sc * (D + 2)], l = recs[(size_t)sc * (D + 2) + 1];
        if (s >= nsplit) { m = -INFINITY; l = 0.f; }
        const float mx = wave_max(m);
        const float w = (m == -INFINITY) ? 0.f : __expf(m - mx);
        const float tot = wave_sum(w * l);
        w_s[s] = w;
        if (s == 0) inv_l = tot > 0.f ? 1.0f / tot : 0.f;
    }
    __syncthreads();
    float o = 0.f;
    int s = 0;
    for (; s + 8 <= nsplit; s += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = recs[(size_t)(s + u) * (D + 2) + 2 + d];
#pragma unroll
        for (int u = 0; u < 8; ++u) o = fmaf(w_s[s + u], v[u], o);
    }
    for (; s < nsplit; ++s) o = fmaf(w_s[s], recs[(size_t)s * (D + 2) + 2 + d], o);
    attn[((size_t)b * hq + h) * D + d] = o * inv_l;
    tls.end();
}

// fused path: grid ((H / rows_per_block) * Hkv, 1, batch), 256 threads.  Every workgroup of a KV head recomputes
// that head's (short-context) attention from L2-resident K/V, then multiplies it with ITS slice of W_o
// (rows_per_block output rows x G*D columns), whose loads were issued before anything else.
template <int D, int G>
__global__ __launch_bounds__(256) void attn_oproj_kernel(unsigned long long* tl, AttnArgs a) {
    const TLStamp tls(tl);
#ifdef PGK_PHASE_STAMPS
    if (threadIdx.x == 0) g_phase_tl = tl;      // same value from every workgroup of the launch
    __syncthreads();
#endif
    constexpr int NWV = 4;   // 8 waves measured slower: the kernel is issue-bound per SIMD, not per wave
    constexpr int LPR = D / 8, PPW = 64 / LPR, RS = D + 2;
    constexpr int GD = G * D, LPW = GD / 8;          // lanes covering one W_o row slice
    constexpr int RPP = NWV * 64 / LPW;              // rows per pass of the workgroup
    constexpr int PRE = 4;                           // preloaded passes
    constexpr int U0 = 12;                           // position-groups per wave in the first KV batch
    __shared__ __attribute__((aligned(16))) float lds[NWV * PPW * G * RS];
    __shared__ __attribute__((aligned(16))) float attn[GD];
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), sub = lane % LPR;   // wid in an SGPR: per-wave branches stay scalar
    // XCD-aware mapping: workgroups are dealt round-robin over the 8 XCDs in linear order, so with the kv head as the
    // FASTEST index all row slices of kv head h land on XCD h % 8 and its K/V rows are fetched into ONE L2 instead of eight
    // (PMC: 9.6 MB of HBM traffic per launch for 4.9 MB of algorithmic bytes with the row slice fastest).  Speed only.
    const int kvh = blockIdx.x % a.hkv, rb = blockIdx.x / a.hkv, b = blockIdx.z;
    const int r0 = rb * a.rows_per_block;
    const int lr = threadIdx.x % LPW, rip = threadIdx.x / LPW;
    const int npass = a.rows_per_block / RPP;
    const bf16* wbase = a.w_o + (size_t)kvh * GD + lr * 8;
    const int ldw = a.hq * D;
    // Issue order = arrival order (vector memory returns in order): first the few L2-resident bytes the new token's
    // q/k/v need, then the cached K/V rows, last the W_o slice that is only consumed at the very end.  (The first
    // version issued W_o and K/V first: the q/k/v row then arrived behind ~1.4 KiB per lane of HBM traffic and the
    // norm / RoPE work started 2.9 us into the workgroup - in-kernel stamps, tools/phase_stamps.py.)
    const size_t head_off = (((size_t)b * a.hkv + kvh) * a.max_seq) * D;
    uint4 pre[PRE];
    KVBatch<U0> kb0;
    NewTokenRaw<G> raw;
    new_token_load<D, G>(a, b, kvh, lane, raw);
    __builtin_amdgcn_sched_barrier(0);
    // first KV batch: U0 position-groups per wave = positions [0, U0*NWV*PPW); addresses do not depend on
    // the context length (clamped), so these loads share the round trip of everything else in this kernel
    kv_issue<D, U0, NWV>(kb0, a.kcache + head_off, a.vcache + head_off, wid * PPW, a.max_seq - 1, lane);
#pragma unroll
    for (int p = 0; p < PRE; ++p)  // unconditional (clamped) so nothing waits on these until the GEMV
        pre[p] = load_nt16(wbase + (size_t)(r0 + min(p, npass - 1) * RPP + rip) * ldw);
    __builtin_amdgcn_sched_barrier(0);
    const int pos = load_uniform_i32(a.positions + b);     // scalar path: not queued behind the 50-odd vector loads above
    tls.phase(0);
    NewToken<D, G> t;
    new_token_finish<D, G>(a, lane, raw, t);
    if (rb == 0 && pos < a.max_seq && wid == 0 && lane < LPR) {
        *reinterpret_cast<uint4*>(a.kcache + head_off + (size_t)pos * D + sub * 8) = t.kbits;
        *reinterpret_cast<uint4*>(a.vcache + head_off + (size_t)pos * D + sub * 8) = t.vbits;
    }
    tls.phase(1);
    DecodeState<G> st;
    st.init();
    const int c1 = min(pos, a.max_seq);
    kv_consume<D, G, U0, NWV>(kb0, wid * PPW, c1, t.qb, lane, st);
    if (c1 > U0 * NWV * PPW)
        decode_walk_trips<D, G, 8, NWV>(a.kcache + head_off, a.vcache + head_off, U0 * NWV * PPW, c1, t.qb, lane, wid, st);
    if (wid == 0 && lane < LPR) fold_new_token<D, G>(t, st);
    tls.phase(2);
    decode_block_merge_lds<D, G, NWV>(st, lds, attn, lane, wid);
    tls.phase(3);

    float xf[8];
    {
        const float4 u = *reinterpret_cast<const float4*>(attn + lr * 8), v = *reinterpret_cast<const float4*>(attn + lr * 8 + 4);
        xf[0] = u.x; xf[1] = u.y; xf[2] = u.z; xf[3] = u.w; xf[4] = v.x; xf[5] = v.y; xf[6] = v.z; xf[7] = v.w;
    }
    float* outp = a.opart + ((size_t)b * a.hkv + kvh) * a.H;
    for (int p = 0; p < npass; ++p) {
        const int row = r0 + p * RPP + rip;
        uint4 w = (p < PRE) ? pre[p < PRE ? p : 0] : load_nt16(wbase + (size_t)row * ldw);
        float wf[8];
        WTraits<bf16>::decode(w, wf);
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc = fmaf(wf[j], xf[j], acc);
        acc = group_sum<LPW>(acc);
        if (lr == 0) outp[row] = acc;
    }
    tls.phase(4);
    tls.end();
}

// ---------------------------------------------------------------------------------------------------------------------
// Fused batch-1 attention + o_proj with both products on the matrix pipe (head_dim 128).
//
// attn_oproj_kernel above spends 2.1 of its 5.5 us in the score / P.V loop: one wave per SIMD, ~750 VALU instructions per 48
// positions (v_dot2c at ~10 cycles of issue, DPP reductions).  The first attempt to move Q.K^T to MFMA loaded the K rows
// from global memory in A-fragment shape (lane = row): 64 separate 16-byte pieces per instruction, and the kernel lost
// more in its load issue phase than the MFMAs won.  Here the cached rows are staged ROW-MAJOR by LDS-DMA -
// the same bytes per instruction as the register loads they replace, 1 KiB contiguous each - and the fragments come out
// of LDS: the one-tile prefill kernel's scheme (ops_attention.hip, attn_short_kernel) with the G query heads of the kv
// head as the only live columns:
//   * chunks of 192 positions: K and V rows [c0, c0 + 192) -> LDS (K: 16-byte chunks XOR row & 15; V: layout (b) of the
//     CDNA guide for ds_read_b64_tr_b16); chunk 0 is requested before the position is known (clamped rows),
//     a later chunk by live tiles only;
//   * wave w takes tiles w, w + 4, w + 8 of the chunk (16 positions each): S^T = K.Q^T - rows = positions, columns =
//     heads - so a lane holds ONE head's scores of 4 consecutive positions per tile; max / sum are lane-local + two
//     shuffles; exp'd and packed to bf16 they are the B operand of O^T = V^T.P^T with no LDS round trip (k-slot j of lane
//     quarter q <-> position 16 tile(j >> 2) + 4 q + (j & 3), V read with the same slots through the transposing read);
//   * every wave keeps a running (m, l, O^T) across chunks; at the end the four waves' states and the new token's
//     (score, 1, v) meet in LDS and are combined per output element, then the W_o slice product as before.
// The new token's k/v never enter the LDS images (the DMA of its cache row would race the write): it is a fifth partial.
// AM_CHUNK = 192 positions per staged chunk (12 tiles, 3 per wave): attn_tail_plan.h, with the live-tile and wait-count
// arithmetic of the request order.

// s_waitcnt takes an immediate: a counted wait whose count depends on the context picks among the few legal ones with a
// wave-uniform branch (am_wait_vm_tiles: 4 per live tile)
template <int N>
__device__ __forceinline__ void am_wait_vm() {
    static_assert(N >= 0 && N <= 63, "vmcnt holds 6 bits");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
template <int (*COUNT)(int)>
__device__ __forceinline__ void am_wait_vm_tiles(int n) {
    if (n >= 3) am_wait_vm<COUNT(3)>();
    else if (n == 2) am_wait_vm<COUNT(2)>();
    else if (n == 1) am_wait_vm<COUNT(1)>();
    else am_wait_vm<COUNT(0)>();
}

__device__ __forceinline__ int am_koff(int row, int ch) { return row * 256 + ((ch ^ (row & 15)) << 4); }
__device__ __forceinline__ int am_voff(int row, int ch) { return row * 256 + ((ch ^ (((row & 3) << 2) | ((row >> 2) & 3))) << 4); }

// OPROJ = false: the whole-context BATCH attention (one workgroup per (sequence, kv head), grid (Hkv, 1, batch)): the same
// kernel without the W_o slice - the normalised heads leave as bf16 (attn_direct16) or fp32 (attn_direct) rows.
//
// The 14 dwords the dispatcher preloads into SGPRs (Makefile) are the LEADING arguments: everything the new token's requests
// and the K requests of chunk 0 need - the step's qkv rows, this layer's K cache, the RoPE rows, the two gammas, and the two
// integers every offset is made of (hq = G * hkv; the qkv row is (hq + 2 hkv) * 128 floats; launch_attn_mfma checks both
// against the struct).  The timeline pointer follows them (TLStamp's deferred form), then the struct, whose scalar fetch
// through the cache the dispatch just invalidated completes under the 12 + NRAW requests that do not need it; its first
// consumers are the position load, the V requests and the W_o preloads.
// Grid: fused form (Hkv, H / rows_per_block, 1) - kv head in x, row slice in y: no division, and the linear workgroup id
// (kv head fastest: XCD-aware, attn_oproj_kernel) is what it was; batch form (Hkv, 1, B).
template <int G, bool OPROJ = true>
__global__ __launch_bounds__(256) void attn_oproj_mfma_kernel(const float* qkv_, bf16* kcache_, const float* rope_cos_, const float* rope_sin_,
                                                              const bf16* q_gamma_, const bf16* k_gamma_, int hkv_, int max_seq_,
                                                              unsigned long long* tl, AttnArgs a) {
    const TLStamp tls(tl, TLStamp::Deferred{});
    typedef __bf16 am_bf16x8 __attribute__((ext_vector_type(8)));
    typedef float am_f32x4 __attribute__((ext_vector_type(4)));
    typedef short am_v4s __attribute__((ext_vector_type(4)));
    constexpr int D = 128, NWV = 4, LPR = 16, RS = D + 4;   // a state record: o[128], then m, l (16-byte aligned rows)
    constexpr int GD = G * D, LPW = GD / 8, RPP = NWV * 64 / LPW, PRE = OPROJ ? 4 : 0;
    extern __shared__ __attribute__((aligned(16))) char am_lds[];          // K image | V image (AM_CHUNK rows x 256 bytes each)
    char* k_lds = am_lds;
    char* v_lds = am_lds + AM_CHUNK * 256;
    __shared__ __attribute__((aligned(16))) float part[NWV + 1][G][RS];    // (o[128], m, l) of the four waves + the new token
    __shared__ __attribute__((aligned(16))) float attn[GD];
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, q4 = lane >> 4;
    const int kvh = blockIdx.x, rb = blockIdx.y, b = blockIdx.z;
    const int hq = G * hkv_;
    const int lr = threadIdx.x % LPW, rip = threadIdx.x / LPW;
    const size_t head_off = (((size_t)b * hkv_ + kvh) * max_seq_) * D;
    const bf16* kc = kcache_ + head_off;

    // Issue order = arrival order, and every wait on it is written out here: the new token's inputs, the cache chunk and
    // nothing else go through LDS-DMA issued as inline asm, so the compiler neither counts them nor - as it does for the
    // builtin form - answers any vector load older than them with vmcnt(0) (which made the norm / RoPE work wait for
    // the whole chunk).  Per wave: NRAW instructions for ITS copy of the new token's fp32 q/k/v slices, the two gammas
    // and the RoPE row (3 KiB for G = 2: three instructions instead of 14 register loads), 24 for the chunk, then the four
    // W_o preloads as ordinary loads.
    constexpr int HB = (G + 2) * 512;                     // bytes of the head slices in a wave's slot; then gq, gk, cos, sin (256 each)
    constexpr int NRAW = (HB + 1024 + 1023) / 1024;
    __shared__ __attribute__((aligned(16))) char raw_lds[NWV][NRAW * 1024];
    // Where it can, a request uses the scalar-base form (lds_dma16_so): no 64-bit address arithmetic per lane.  Every base
    // here is made on the scalar unit from kernel arguments and workgroup ids (no VALU-written SGPR feeds it).
    {
        const char* row = reinterpret_cast<const char*>(qkv_ + (size_t)b * ((hq + 2 * hkv_) * D));
        const char* cosr = reinterpret_cast<const char*>(rope_cos_ + (size_t)b * 64);
        const char* sinr = reinterpret_cast<const char*>(rope_sin_ + (size_t)b * 64);
        const char* gqp = q_gamma_ ? reinterpret_cast<const char*>(q_gamma_) : cosr;      // no QK-norm: any valid bytes
        const char* gkp = k_gamma_ ? reinterpret_cast<const char*>(k_gamma_) : cosr;
        auto head_byte = [&](int hs) { return (uint32_t)((hs < G) ? (kvh * G + hs) * D : (hs == G ? (hq + kvh) * D : (hq + hkv_ + kvh) * D)) * 4u; };
#pragma unroll
        for (int i = 0; i < NRAW; ++i) {
            const int o = 1024 * i + 16 * lane;
            if (1024 * (i + 1) <= HB) {                   // two whole head slices: the qkv row is the scalar base
                const uint32_t within = (uint32_t)(16 * lane) & 511u;
                lds_dma16_so(row, (lane < 32 ? head_byte(2 * i) : head_byte(2 * i + 1)) + within, lds_addr_of(&raw_lds[wid][0]) + 1024 * i);
            } else {
                const char* src;
                if (o < HB) {
                    src = row + head_byte(o >> 9) + (o & 511);
                } else {
                    const int o2 = min(o - HB, 1023), seg = o2 >> 8, within = o2 & 255;
                    src = (seg == 0 ? gqp : seg == 1 ? gkp : seg == 2 ? cosr : sinr) + within;
                }
                lds_dma16(src, lds_addr_of(&raw_lds[wid][0]) + 1024 * i);
            }
        }
    }
    // The chunk, WAVE-OWNED: wave w requests the rows of the tiles it consumes - tiles w, w + 4, w + 8 (16 rows each), every
    // tile in four instructions of 4 rows: instruction (u, r) covers chunk rows rl = 16 (w + 4 u) + 4 r + q4, lane (q4, l15)
    // fetching 16-byte piece l15 ^ swizzle(rl) of its row (K: rl & 15 = 4 r + q4; V: ((rl & 3) << 2) | ((rl >> 2) & 3) =
    // 4 q4 + r - neither depends on w or u) into LDS row rl.  So a lane's byte offset from row c0 of the head is
    //   off(u, r) = koff[r] + 16384 u,   koff[r] = 4096 w + 1024 r + 256 q4 + 16 (l15 ^ swizzle):
    // four values per image made once; the step over u is a scalar add to the base.  No wave reads another wave's rows of
    // the images, so no barrier stands between a wave's requests and its own reads - only its own counted waits.
    // The clamp.  A request must stay inside the head's max_seq rows.  (a) c0 + AM_CHUNK <= max_seq (wave-uniform): every
    // row c0 + rl, rl < AM_CHUNK, is a cache row - no clamp.  (b) otherwise the row is min(c0 + rl, max_seq - 1) as before,
    // taken on the 32-bit byte offsets: off = 256 rl + s and lim = 256 (max_seq - 1 - c0) + s carry the same s < 256, so
    // min(off, lim) = 256 min(rl, max_seq - 1 - c0) + s, and c0 <= max_seq - 1 wherever a chunk is staged (c0 = 0, or
    // c0 < c1 <= max_seq).  Offsets stay below 256 max_seq: 32 bits hold them for any cache under 16 M rows.  Clamped
    // rows are fetched and masked (positions >= c1 never count), as they always were.
    uint32_t koff[4], voff[4];
    {
        const uint32_t wq = ((threadIdx.x >> 6) << 12) | ((uint32_t)q4 << 8);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            koff[r] = wq + 1024 * r + ((uint32_t)(l15 ^ (4 * r + q4)) << 4);
            voff[r] = wq + 1024 * r + ((uint32_t)(l15 ^ (4 * q4 + r)) << 4);
        }
    }
    static_assert(AM_CHUNK == 16 * 3 * NWV, "a chunk is three 16-row tiles per wave: 12 K and 12 V requests per wave");
    constexpr int NREQ = AM_CHUNK / 4 / NWV;              // requests per wave and image
    // ntile: the wave's first ntile tiles only (wave-uniform; chunk 0: the constant 3) - its last row is below c0 + 64 ntile,
    // which is what (a) asks of the cache.
    auto stage_image = [&](const bf16* head, const uint32_t (&off)[4], uint32_t lds_img, int c0, int ntile) {
        const bf16* base = head + (size_t)c0 * D;
        const uint32_t dst = lds_img + wid * 4096;
        if (c0 + 64 * ntile <= max_seq_) {                // (a)
#pragma unroll
            for (int u = 0; u < 3; ++u)
                if (u < ntile) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) lds_dma16_so(base + u * 64 * D, off[r], dst + u * 16384 + r * 1024);
                }
        } else {                                          // (b)
            const uint32_t last = (uint32_t)(max_seq_ - 1 - c0) << 8;
#pragma unroll
            for (int u = 0; u < 3; ++u)
                if (u < ntile) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) lds_dma16_so(base, min(off[r] + 16384u * u, last | (off[r] & 0xF0u)), dst + u * 16384 + r * 1024);
                }
        }
    };
    stage_image(kc, koff, lds_addr_of(k_lds), 0, 3);
    __builtin_amdgcn_sched_barrier(0);
    // From here on the struct.  The position first: read through the constant address space it is a scalar load the compiler
    // counts itself - issued here, ahead of the V requests, waited for where the value is first used (positions[] is not
    // written by this launch, and the dispatch invalidated the scalar cache, which load_uniform_i32 relies on too).
    const int pos = *(const __attribute__((address_space(4))) int32_t*)(a.positions + b);
    const bf16* vc = a.vcache + head_off;
    stage_image(vc, voff, lds_addr_of(v_lds), 0, 3);
    const int r0 = rb * a.rows_per_block;
    const int npass = a.rows_per_block / RPP;
    const bf16* wbase = a.w_o + (size_t)kvh * GD + lr * 8;
    const int ldw = hq * D;
    uint4 pre[PRE > 0 ? PRE : 1];
#pragma unroll
    for (int p = 0; p < PRE; ++p) pre[p] = load_nt16(wbase + (size_t)(r0 + min(p, npass - 1) * RPP + rip) * ldw);
    __builtin_amdgcn_sched_barrier(0);
    tls.phase(0);
    // Vector memory returns in issue order, and per wave that order is: NRAW new-token requests, NREQ K, NREQ V, PRE W_o
    // loads.  A wait for "at most n outstanding" therefore means: everything but the n youngest has landed.  The counts are
    // attn_tail_plan.h's: am_wait_new = the whole chunk + W_o, am_wait_k0 = chunk 0's V rows + W_o, am_wait_v0 = W_o; later
    // chunks (W_o long landed - it is older) am_wait_k = the V rows of the wave's live tiles, then 0.
    static_assert(NREQ == 3 * AM_TILE_REQ && am_wait_new(PRE) == 2 * NREQ + PRE && am_wait_k0(PRE) == NREQ + PRE && am_wait_v0(PRE) == PRE &&
                      am_wait_k(3) == NREQ && am_wait_k(2) == 8 && am_wait_k(1) == 4 && am_wait_k(0) == 0,
                  "wait counts follow the request order above");
    am_wait_vm<am_wait_new(PRE)>();
    // The new token's G + 2 head vectors (q heads, k, v) are SPLIT over the waves - item i goes to wave i % 4 - instead of
    // every wave normalising and rotating all of them (0.74 us of ALU per wave in attn_oproj_kernel): each wave reads its
    // item from its own copy of the inputs, and the results meet in LDS behind the barrier that the cache chunk needs anyway.
    __shared__ __attribute__((aligned(16))) uint4 q_sh[G][16], k_sh[16], v_sh[16];   // bf16, 16 chunks of 8 dims per vector
    {
        const char* slot = &raw_lds[wid][0];
        const int sub = l15;                                 // the lane's 8 dims: sub * 8 .. + 8 (all four lane quarters compute the same)
        const int dd = (sub * 8) % 64;
        float csv[8], snv[8];
        {
            const float4 c0v = *reinterpret_cast<const float4*>(slot + HB + 512 + dd * 4), c1v = *reinterpret_cast<const float4*>(slot + HB + 512 + dd * 4 + 16);
            const float4 s0v = *reinterpret_cast<const float4*>(slot + HB + 768 + dd * 4), s1v = *reinterpret_cast<const float4*>(slot + HB + 768 + dd * 4 + 16);
            csv[0] = c0v.x; csv[1] = c0v.y; csv[2] = c0v.z; csv[3] = c0v.w; csv[4] = c1v.x; csv[5] = c1v.y; csv[6] = c1v.z; csv[7] = c1v.w;
            snv[0] = s0v.x; snv[1] = s0v.y; snv[2] = s0v.z; snv[3] = s0v.w; snv[4] = s1v.x; snv[5] = s1v.y; snv[6] = s1v.z; snv[7] = s1v.w;
        }
        const bool has_norm = q_gamma_ != nullptr;
        for (int item = wid; item < G + 2; item += NWV) {    // wave-uniform
            const float4 lo = *reinterpret_cast<const float4*>(slot + item * 512 + sub * 32), hi = *reinterpret_cast<const float4*>(slot + item * 512 + sub * 32 + 16);
            float x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            if (item < G + 1) {                              // q heads and k: QK-norm (optional) + RoPE, the arithmetic of new_token_finish
                if (has_norm) {
                    float gm[8];
                    WTraits<bf16>::decode(*reinterpret_cast<const uint4*>(slot + HB + (item < G ? 0 : 256) + sub * 16), gm);
                    float ss = 0.f;
#pragma unroll
                    for (int j = 0; j < 8; ++j) ss = fmaf(x[j], x[j], ss);
                    ss = group_sum<LPR>(ss);
                    const float inv = 1.0f / sqrtf(ss / D + a.eps);
#pragma unroll
                    for (int j = 0; j < 8; ++j) x[j] = x[j] * inv * gm[j];
                }
                const bool lo_half = sub < LPR / 2;
                float o8[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float other = xor_half<LPR>(x[j]);
                    o8[j] = lo_half ? (x[j] * csv[j] - other * snv[j]) : (x[j] * csv[j] + other * snv[j]);
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] = (item < G) ? o8[j] * a.scale : o8[j];
            }
            Vec<bf16> vb;
            vb.from_float(x);
            if (lane < 16) {
                if (item < G) q_sh[item][lane] = vb.raw;
                else if (item == G) k_sh[lane] = vb.raw;
                else v_sh[lane] = vb.raw;
            }
        }
    }
    tls.phase(1);
    const int c1 = min(pos, max_seq_);                  // cached positions [0, c1)
    uint4 qf[4];
    float m_run = -INFINITY, l_run = 0.f;                // of head l15 (lanes l15 >= G carry dummies)
    am_f32x4 o[D / 16];
#pragma unroll
    for (int i = 0; i < D / 16; ++i) o[i] = am_f32x4{0.f, 0.f, 0.f, 0.f};
    const int tq = l15 >> 2, tp = l15 & 3;
    for (int c0 = 0; c0 == 0 || c0 < c1; c0 += AM_CHUNK) {
        if (c0 > 0) {
            // The position is long known: a wave requests only its live tiles - the test the consumer below makes - so a
            // context that ends early in the chunk costs the requests of what it holds, not 24 per wave (context 194 against
            // 190: +48 us per step before).  Rows of a live tile at or past c1 are fetched and masked as ever.
            // Dead tiles keep the previous chunk's rows: finite cache rows under weights of zero, as the clamped rows were.
            // no barrier: a wave overwrites only the image rows it alone reads, and its reads of the previous chunk have
            // returned (their values went through the MFMAs above; the asm statements keep the compiler's order)
            const int nlive = __builtin_amdgcn_readfirstlane(am_live_tiles(c0, c1, wid));
            stage_image(kc, koff, lds_addr_of(k_lds), c0, nlive);
            stage_image(vc, voff, lds_addr_of(v_lds), c0, nlive);
            am_wait_vm_tiles<am_wait_k>(nlive);
        } else {
            __syncthreads();                               // publishes q_sh / k_sh / v_sh; in front of the waits, so no wave idles at it with its rows landed
            am_wait_vm<am_wait_k0(PRE)>();
        }
        __builtin_amdgcn_sched_barrier(0);
        if (c0 == 0) {
            // q as B fragments: lane (l15 = head, q4) of k-step ks holds dims 32 ks + 8 q4 .. + 8 of head l15
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const uint4 v = q_sh[min(l15, G - 1)][4 * ks + q4];
                qf[ks] = l15 < G ? v : make_uint4(0, 0, 0, 0);
            }
            // the new token: fifth partial (score = q . k_new per head, weight 1, value v_new) - the last wave, which had the
            // fewest items above (its cache row is stored behind the chunk loop: a store between the requests and their
            // counted waits would be one more operation in the count)
            if (wid == NWV - 1 && lane < LPR) {
                float kn[8], vn[8];
                Vec<bf16> kb, vb2;
                kb.raw = k_sh[lane]; vb2.raw = v_sh[lane];
                kb.to_float(kn); vb2.to_float(vn);
                const bool live = pos < max_seq_;
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    Vec<bf16> qb;
                    qb.raw = q_sh[g][lane];
                    float qv[8];
                    qb.to_float(qv);
                    float dsum = 0.f;
#pragma unroll
                    for (int j = 0; j < 8; ++j) dsum = fmaf(qv[j], kn[j], dsum);
                    dsum = group_sum<LPR>(dsum);
                    if (lane == 0) { part[NWV][g][D] = live ? dsum : -INFINITY; part[NWV][g][D + 1] = live ? 1.f : 0.f; }
#pragma unroll
                    for (int j = 0; j < 8; ++j) part[NWV][g][lane * 8 + j] = vn[j];
                }
            }
        }
        // S^T tiles of this wave: rows = positions c0 + 16 t + 4 q4 + r, column = head l15
        am_f32x4 s[3];
        float mx = -INFINITY;
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int tile = wid + NWV * u;
            s[u] = am_f32x4{0.f, 0.f, 0.f, 0.f};
            if (c0 + 16 * tile < c1) {                     // wave-uniform
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const uint4 ka = *reinterpret_cast<const uint4*>(k_lds + am_koff(16 * tile + l15, 4 * ks + q4));
                    s[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(am_bf16x8, ka), __builtin_bit_cast(am_bf16x8, qf[ks]), s[u], 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool ok = c0 + 16 * tile + 4 * q4 + r < c1;
                s[u][r] = ok ? s[u][r] : -INFINITY;
                mx = fmaxf(mx, s[u][r]);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const float alpha = (m_new == -INFINITY) ? 1.f : __expf(m_run - m_new);
        float ls = 0.f;
        uint32_t pk[3][2];
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            float p[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) p[r] = (m_new == -INFINITY) ? 0.f : __expf(s[u][r] - m_new);
            pk[u][0] = pack_bf16x2(p[0], p[1]);
            pk[u][1] = pack_bf16x2(p[2], p[3]);
            ls += (__uint_as_float(pk[u][0] << 16) + __uint_as_float(pk[u][0] & 0xFFFF0000u)) + (__uint_as_float(pk[u][1] << 16) + __uint_as_float(pk[u][1] & 0xFFFF0000u));
        }
        ls += __shfl_xor(ls, 16, 64);
        ls += __shfl_xor(ls, 32, 64);
        l_run = l_run * alpha + ls;
        m_run = m_new;
#pragma unroll
        for (int i = 0; i < D / 16; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[i][r] *= alpha;
        // O^T += V^T . P^T: step 0 pairs tiles (wid, wid + 4), step 1 tile wid + 8 with zeros - all three this wave's own requests
        if (c0 > 0) am_wait_vm<0>();
        else am_wait_vm<am_wait_v0(PRE)>();
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int st2 = 0; st2 < 2; ++st2) {
            const int ta = wid + NWV * (2 * st2), tb = (st2 == 0) ? wid + NWV : ta;     // tb of step 1: any staged tile (weights zero)
            if (c0 + 16 * ta < c1) {                       // wave-uniform
                const uint4 pf = make_uint4(pk[2 * st2][0], pk[2 * st2][1], st2 == 0 ? pk[1][0] : 0u, st2 == 0 ? pk[1][1] : 0u);
                const int ra = 16 * ta + 4 * q4 + tq, rbv = 16 * tb + 4 * q4 + tq;
#pragma unroll
                for (int i = 0; i < D / 16; ++i) {
                    const am_v4s a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) am_v4s*)(v_lds + am_voff(ra, 2 * i + (tp >> 1)) + 8 * (tp & 1)));
                    const am_v4s a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) am_v4s*)(v_lds + am_voff(rbv, 2 * i + (tp >> 1)) + 8 * (tp & 1)));
                    const uint2 u0 = __builtin_bit_cast(uint2, a0), u1 = __builtin_bit_cast(uint2, a1);
                    const uint4 va = make_uint4(u0.x, u0.y, u1.x, u1.y);
                    o[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(am_bf16x8, va), __builtin_bit_cast(am_bf16x8, pf), o[i], 0, 0, 0);
                }
            }
        }
    }
    tls.phase(2);
    if (rb == 0 && wid == NWV - 1 && lane < LPR && pos < max_seq_) {     // the new token's cache row (k_sh / v_sh: read-only since the barrier)
        *reinterpret_cast<uint4*>(kcache_ + head_off + (size_t)pos * D + lane * 8) = k_sh[lane];
        *reinterpret_cast<uint4*>(a.vcache + head_off + (size_t)pos * D + lane * 8) = v_sh[lane];
    }
    // the waves' states -> LDS: lane (l15 = head g, q4) holds dims 16 i + 4 q4 + r of head g
    if (l15 < G) {
        if (q4 == 0) { part[wid][l15][D] = m_run; part[wid][l15][D + 1] = l_run; }
#pragma unroll
        for (int i = 0; i < D / 16; ++i)
            *reinterpret_cast<float4*>(&part[wid][l15][16 * i + 4 * q4]) = make_float4(o[i][0], o[i][1], o[i][2], o[i][3]);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < GD; e += 256) {
        const int g = e / D, d = e % D;
        float mstar = -INFINITY;
#pragma unroll
        for (int w = 0; w <= NWV; ++w) mstar = fmaxf(mstar, part[w][g][D]);
        float num = 0.f, den = 0.f;
#pragma unroll
        for (int w = 0; w <= NWV; ++w) {
            const float mw = part[w][g][D];
            const float wgt = (mw == -INFINITY) ? 0.f : __expf(mw - mstar);
            num = fmaf(wgt, part[w][g][d], num);
            den = fmaf(wgt, part[w][g][D + 1], den);
        }
        attn[e] = den > 0.f ? num / den : 0.f;
    }
    __syncthreads();
    tls.phase(3);
    if constexpr (OPROJ) {
        float xf[8];
        {
            const float4 u = *reinterpret_cast<const float4*>(attn + lr * 8), v = *reinterpret_cast<const float4*>(attn + lr * 8 + 4);
            xf[0] = u.x; xf[1] = u.y; xf[2] = u.z; xf[3] = u.w; xf[4] = v.x; xf[5] = v.y; xf[6] = v.z; xf[7] = v.w;
        }
        float* outp = a.opart + ((size_t)b * a.hkv + kvh) * a.H;
        // The pass counts the engine's row slicing produces (at most PRE preloaded passes per workgroup) as compile-time
        // constants: fully unrolled, pre[] read with static indices (registers, no indexing through memory), and the NP
        // independent cross-lane sums next to each other for the scheduler to interleave.  Per pass the same eight FMAs
        // and the same reduction as the runtime loop below, which stays for any other slicing.
        auto wo_fixed = [&](auto np_c) {
            constexpr int NP = decltype(np_c)::value;
            static_assert(NP <= PRE, "every pass of a fixed count is preloaded");
            float acc[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                float wf[8];
                WTraits<bf16>::decode(pre[p], wf);
                acc[p] = 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[p] = fmaf(wf[j], xf[j], acc[p]);
            }
#pragma unroll
            for (int p = 0; p < NP; ++p) acc[p] = group_sum<LPW>(acc[p]);
            if (lr == 0) {
#pragma unroll
                for (int p = 0; p < NP; ++p) outp[r0 + p * RPP + rip] = acc[p];
            }
        };
        if (npass == 4) wo_fixed(std::integral_constant<int, 4>{});
        else if (npass == 2) wo_fixed(std::integral_constant<int, 2>{});
        else if (npass == 1) wo_fixed(std::integral_constant<int, 1>{});
        else {
            for (int p = 0; p < npass; ++p) {
                const int row = r0 + p * RPP + rip;
                uint4 w = (p < PRE) ? pre[p < PRE ? p : 0] : load_nt16(wbase + (size_t)row * ldw);
                float wf[8];
                WTraits<bf16>::decode(w, wf);
                float acc = 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) acc = fmaf(wf[j], xf[j], acc);
                acc = group_sum<LPW>(acc);
                if (lr == 0) outp[row] = acc;
            }
        }
    } else {
        const size_t ob = ((size_t)b * a.hq + (size_t)kvh * G) * D;
        if (a.attn_direct16) {
            for (int e = threadIdx.x; e < GD; e += 256) a.attn_direct16[ob + e] = from_f<bf16>(attn[e]);
        } else {
            for (int e = threadIdx.x; e < GD; e += 256) a.attn_direct[ob + e] = attn[e];
        }
    }
    tls.phase(4);
    tls.end();
}

// long-context path, steps 2 + 3 in ONE launch: merge the split-KV records of a kv head's G query heads (the arithmetic
// of attn_merge_kernel, same order) and multiply the result with this workgroup's slice of W_o.  Grid as attn_oproj_kernel
// ((H / rows_per_block) * Hkv, kv head fastest: XCD-aware), output the same per-kv-head partial vectors, which the
// gate/up kernel's PRO_NORM_SUM prologue adds to the residual stream.  Replaces attn_merge_kernel + the o_proj GEMV:
// one launch and one dependent-kernel gap less per layer (context 2048, w8a16: the pair took 1.95 + 1.3 + 1.74 us of
// every 23.8 us layer; profiles/r02_config3_timeline.json).  W_o bf16 or fp8 (16 codes per lane, block scale in registers).
template <int D, int G, bool FP8>
__global__ __launch_bounds__(256) void attn_merge_oproj_kernel(unsigned long long* tl, AttnArgs a) {
    const TLStamp tls(tl);
    constexpr int RS = D + 2, GD = G * D;
    constexpr int NWT = FP8 ? 16 : 8;                // weights per 16-byte load
    constexpr int LPW = GD / NWT;                    // lanes covering one W_o row slice
    constexpr int RPP = 256 / LPW;                   // rows per pass of the workgroup
    constexpr int PRE = 4;
    static_assert(LPW <= 64 && 256 % LPW == 0, "row slice must fit a wave");
    __shared__ float w_s[G][64];
    __shared__ float inv_l[G];
    __shared__ __attribute__((aligned(16))) float attn[GD];
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int kvh = blockIdx.x % a.hkv, rb = blockIdx.x / a.hkv, b = blockIdx.z;
    const int r0 = rb * a.rows_per_block;
    const int lr = threadIdx.x % LPW, rip = threadIdx.x / LPW;
    const int npass = a.rows_per_block / RPP;
    const int ldw = a.hq * D;
    const int col0 = kvh * GD + lr * NWT;
    const char* wbase = reinterpret_cast<const char*>(a.w_o) + (size_t)col0 * (FP8 ? 1 : 2);
    const size_t row_bytes = (size_t)ldw * (FP8 ? 1 : 2);
    // the record words first (L2, written by the launch before), then the W_o stream: arrival order = issue order
    const float* hrecs = a.part + ((size_t)b * a.hq + (size_t)kvh * G) * a.nsplit * RS;
    float m = -INFINITY, l = 0.f;
    if (wid < G) {
        const int sc = min(lane, a.nsplit - 1);
        m = hrecs[((size_t)wid * a.nsplit + sc) * RS];
        l = hrecs[((size_t)wid * a.nsplit + sc) * RS + 1];
    }
    // ... and the records' value words of this thread's output element(s): up to 32 slices per element straight into
    // registers, BEFORE the W_o stream and before the barrier below.  (They used to be read after the barrier, eight at a
    // time: three to four dependent L2 round trips on the critical path of every layer at context 2048.)
    constexpr int EPT = (GD + 255) / 256, RPRE = 32;
    float rv[EPT][RPRE];
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const int e = min((int)threadIdx.x + 256 * i, GD - 1), g = e / D, d = e % D;
        const float* recs = hrecs + (size_t)g * a.nsplit * RS + 2 + d;
#pragma unroll
        for (int u = 0; u < RPRE; ++u) rv[i][u] = recs[(size_t)min(u, a.nsplit - 1) * RS];
    }
    __builtin_amdgcn_sched_barrier(0);
    uint4 pre[PRE];
    float psc[PRE];
#pragma unroll
    for (int p = 0; p < PRE; ++p) {
        const int row = r0 + min(p, npass - 1) * RPP + rip;
        pre[p] = load_nt16(wbase + (size_t)row * row_bytes);
        if constexpr (FP8) psc[p] = to_f(a.w_o_scale[(size_t)(row >> 7) * (ldw >> 7) + (col0 >> 7)]);
    }
    __builtin_amdgcn_sched_barrier(0);
    tls.phase(0);
    if (wid < G) {
        if (lane >= a.nsplit) { m = -INFINITY; l = 0.f; }
        const float mx = wave_max(m);
        const float w = (m == -INFINITY) ? 0.f : __expf(m - mx);
        const float tot = wave_sum(w * l);
        w_s[wid][lane] = w;
        if (lane == 0) inv_l[wid] = tot > 0.f ? 1.0f / tot : 0.f;
    }
    __syncthreads();
    tls.phase(1);
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const int e = (int)threadIdx.x + 256 * i;
        if (e < GD) {
            const int g = e / D, d = e % D;
            const float* recs = hrecs + (size_t)g * a.nsplit * RS;
            float o = 0.f;
#pragma unroll
            for (int u = 0; u < RPRE; ++u) o = fmaf(u < a.nsplit ? w_s[g][u] : 0.f, rv[i][u], o);   // same order as attn_merge_kernel
            for (int s2 = RPRE; s2 < a.nsplit; ++s2) o = fmaf(w_s[g][s2], recs[(size_t)s2 * RS + 2 + d], o);
            attn[e] = o * inv_l[g];
        }
    }
    __syncthreads();
    tls.phase(2);
    float xf[NWT];
#pragma unroll
    for (int i = 0; i < NWT / 4; ++i) {
        const float4 u = *reinterpret_cast<const float4*>(attn + lr * NWT + 4 * i);
        xf[4 * i] = u.x; xf[4 * i + 1] = u.y; xf[4 * i + 2] = u.z; xf[4 * i + 3] = u.w;
    }
    float* outp = a.opart + ((size_t)b * a.hkv + kvh) * a.H;
    for (int p = 0; p < npass; ++p) {
        const int row = r0 + p * RPP + rip;
        uint4 w;
        float sc = 1.f;
        if (p < PRE) {
            w = pre[p < PRE ? p : 0];
            if constexpr (FP8) sc = psc[p < PRE ? p : 0];
        } else {
            w = load_nt16(wbase + (size_t)row * row_bytes);
            if constexpr (FP8) sc = to_f(a.w_o_scale[(size_t)(row >> 7) * (ldw >> 7) + (col0 >> 7)]);
        }
        float wf[NWT];
        if constexpr (FP8) WTraits<fp8e4m3>::decode(w, wf);
        else WTraits<bf16>::decode(w, wf);
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < NWT; ++j) acc = fmaf(wf[j], xf[j], acc);
        acc = group_sum<LPW>(acc * sc);      // scale per lane: a row slice of G*D columns may span several 128-column scale blocks
        if (lr == 0) outp[row] = acc;
    }
    tls.end();
}

template <int G, bool OPROJ = true>
static hipError_t launch_attn_mfma(dim3 grid, hipStream_t st, const AttnArgs& a) {
    constexpr int lds = 2 * AM_CHUNK * 256;
    static bool attr = false;
    if (!attr) {
        const hipError_t he = hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_oproj_mfma_kernel<G, OPROJ>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (he != hipSuccess) return he;
        attr = true;
    }
    // what the kernel derives instead of fetching: its GQA group is the whole of G, and the qkv row is q, k, v back to back
    if (a.hq != G * a.hkv || a.g_total != G || a.g_off != 0 || a.qkv_ld != (a.hq + 2 * a.hkv) * 128) return hipErrorInvalidValue;
    // the eight leading arguments fill the 14 preloaded dwords; the timeline pointer is the ninth
    return launch_k<8>(attn_oproj_mfma_kernel<G, OPROJ>, grid, dim3(256), lds, st, a.qkv, a.kcache, a.rope_cos, a.rope_sin, a.q_gamma, a.k_gamma, a.hkv, a.max_seq, a);
}

// f(std::integral_constant<int, G>) for the GQA group sizes the attention kernels are instantiated for
template <class F>
static hipError_t with_group(int G, F f) {
    return G == 1 ? f(std::integral_constant<int, 1>{}) : G == 2 ? f(std::integral_constant<int, 2>{}) : G == 4 ? f(std::integral_constant<int, 4>{}) : hipSuccess;
}

// split-KV slices (DIRECT: the whole context in one workgroup) for G query heads per kv head
template <int D, int G>
static hipError_t launch_attn_decode(bool direct, dim3 grid, hipStream_t st, const AttnArgs& a) {
    return direct ? launch_k(attn_decode_kernel<D, G, true>, grid, dim3(256), 0, st, a) : launch_k(attn_decode_kernel<D, G, false>, grid, dim3(256), 0, st, a);
}

// Which attention kernel a chunk of m sequences launches, over how many split-KV slices, and what follows it: the one
// place where this is decided.  launch_attn_d executes the choice; pgk_engine_attn_plan prints it.
enum AttnKernel { AK_FUSED_MFMA = 0, AK_FUSED_DOT2, AK_DIRECT_MFMA, AK_DIRECT, AK_SPLIT };
enum AttnTail { AT_NONE = 0, AT_MERGE, AT_MERGE_OPROJ_BF16, AT_MERGE_OPROJ_FP8 };
struct AttnChoice { AttnKernel kernel; AttnTail tail; int nsplit, span; bool out_bf16; };
inline AttnChoice attn_choice(const Engine* e, int m, int step_span, const AttnFlags& f) {
    const auto& c = e->cfg;
    const int D = c.head_dim, G = c.num_heads / c.num_kv_heads;
    AttnChoice ch{};
    ch.span = (step_span > 0 && step_span < c.max_seq_len) ? step_span : c.max_seq_len;
    // KV slices per (sequence, kv head): as many as fit ONE wave of workgroups over the chip (a 257th workgroup waits
    // for a free CU and adds a tail: 33 slices x 8 heads measured 5 % slower than 32 at context 2048), never more than
    // the workspace was sized for (e->nsplit: ~64 positions per slice at the full cache length)
    // (batches stream enough KV bytes to want two workgroups per CU: measured 22.1 vs 24.6 us at 8 x 2048 positions)
    int ns = e->cu_count * (m >= 4 ? 2 : 1) / (c.num_kv_heads * m);
    const int ns_cap = ceil_div(ch.span, 64) < e->nsplit ? ceil_div(ch.span, 64) : e->nsplit;     // ~64 positions per slice at least, by the TIER (not the cache: a tier slices alike on every cache)
    ns = ns < 1 ? 1 : (ns > ns_cap ? ns_cap : ns);
    // slices are cut by absolute position in whole position-group steps: launch only as many as the step's context tier needs
    // (the tier, not the cache length: with slices of a 4096-row cache a context of 400 kept 3 of 27 slices busy - 0.671 ms per
    // step against 0.623 on a 1024-row cache)
    ch.nsplit = f.direct ? 1 : ceil_div(ch.span, decode_chunk_len(ch.span, ns, 4 * (64 / (D / 8))));
    ch.out_bf16 = f.direct && f.direct_bf16;
    if (!group_instantiated(G)) ch.kernel = f.direct ? AK_DIRECT : AK_SPLIT;   // head-chunk launches: attn_decode_kernel only
    else if (f.fused) ch.kernel = (D == 128 && e->attn_mfma) ? AK_FUSED_MFMA : AK_FUSED_DOT2;
    else if (f.direct) ch.kernel = (D == 128 && e->attn_mfma && m * (int)c.num_kv_heads <= e->cu_count) ? AK_DIRECT_MFMA : AK_DIRECT;
    else ch.kernel = AK_SPLIT;
    const bool f8 = c.weight_format == 1 || c.weight_format == 2;
    ch.tail = f.merged ? (f8 ? AT_MERGE_OPROJ_FP8 : AT_MERGE_OPROJ_BF16) : ((!f.fused && !f.direct) ? AT_MERGE : AT_NONE);
    return ch;
}

// `fused`: attention + o_proj partials in one kernel (one sequence at short context); `direct`: one workgroup per
// (sequence, kv head) walks the whole (short) context and writes the normalised output - no merge launch; otherwise
// split-KV slices, then `merged` (merge + o_proj partials in one launch) or the merge kernel.  Counts its own launches.
template <int D>
static pgk_status launch_attn_d(const StepCtx& cx, int layer, const AttnFlags& af) {
    const bool fused = af.fused, direct = af.direct;
    Engine* e = cx.e;
    const int b0 = cx.b0, m = cx.M;
    const hipStream_t st = cx.st;
    const auto& c = e->cfg;
    const auto& L = e->layers[layer];
    const int G = c.num_heads / c.num_kv_heads;
    const size_t lofs = (size_t)layer * e->kv_layer_elems() + (size_t)b0 * c.num_kv_heads * c.max_seq_len * c.head_dim;
    AttnArgs a{};
    a.qkv = e->qkv + (size_t)b0 * e->qkv_dim();
    a.qkv_ld = e->qkv_dim();
    a.q_gamma = c.use_qk_norm ? (const bf16*)L.q_norm : nullptr;
    a.k_gamma = c.use_qk_norm ? (const bf16*)L.k_norm : nullptr;
    a.eps = c.norm_eps;
    a.rope_cos = e->cur_cos + (size_t)b0 * (D / 2); a.rope_sin = e->cur_sin + (size_t)b0 * (D / 2);
    a.kcache = e->kcache + lofs; a.vcache = e->vcache + lofs;
    a.positions = e->positions + b0;
    a.hq = c.num_heads; a.hkv = c.num_kv_heads; a.max_seq = c.max_seq_len;
    const AttnChoice pick = attn_choice(e, m, e->step_span, af);
    a.span = pick.span;
    a.scale = 1.0f / sqrtf((float)D);
    a.part = e->part + (size_t)b0 * c.num_heads * e->nsplit * (D + 2);
    a.nsplit = pick.nsplit;
    a.w_o = (const bf16*)L.w_o; a.w_o_scale = (const bf16*)L.s_o; a.H = c.hidden_size; a.rows_per_block = e->oproj_rows;
    a.opart = e->opart ? e->opart + (size_t)b0 * c.num_kv_heads * c.hidden_size : nullptr;
    if (direct) {
        a.attn_direct = e->attnv + (size_t)b0 * c.num_heads * D;
        if (pick.out_bf16) a.attn_direct16 = e->attnv16 + (size_t)b0 * c.num_heads * D;
    }
    dim3 grid = fused ? dim3((c.hidden_size / e->oproj_rows) * c.num_kv_heads, 1, m) : dim3(a.nsplit, c.num_kv_heads, m);
    hipError_t he = hipSuccess;
    a.g_total = G;
    a.g_off = 0;
    if (!group_instantiated(G)) {
        // any other group size (Qwen2.5-7B: 28 / 4 = 7): chunks of 4, 2 and 1 query heads per kv head, one launch each -
        // every chunk re-reads the kv head's K/V rows, which is what the reference's GQA-expanded cache costs for ALL heads
        PGK_REQUIRE(!fused, "engine: fused attention needs a GQA group of 1, 2 or 4");
        for (int off = 0; off < G;) {
            const int gc = head_chunk(G, off);
            a.g_off = off;
            he = with_group(gc, [&](auto g) { return launch_attn_decode<D, decltype(g)::value>(direct, grid, st, a); });
            PGK_CHECK_HIP(he);
            ++*cx.launches;
            off += gc;
        }
    } else {
        he = with_group(G, [&](auto g) {
            constexpr int GG = decltype(g)::value;
            if constexpr (D == 128) {
                if (pick.kernel == AK_FUSED_MFMA) return launch_attn_mfma<GG>(dim3(c.num_kv_heads, c.hidden_size / e->oproj_rows, m), st, a);   // kv head in x, row slice in y
                if (pick.kernel == AK_DIRECT_MFMA) return launch_attn_mfma<GG, false>(dim3(c.num_kv_heads, 1, m), st, a);
            }
            if (pick.kernel == AK_FUSED_DOT2) return launch_k(attn_oproj_kernel<D, GG>, grid, dim3(256), 0, st, a);
            return launch_attn_decode<D, GG>(pick.kernel == AK_DIRECT, grid, st, a);
        });
        PGK_CHECK_HIP(he);
        ++*cx.launches;
    }
    if (pick.tail == AT_MERGE_OPROJ_BF16 || pick.tail == AT_MERGE_OPROJ_FP8) {
        // split-KV merge + o_proj partial products in one launch (attn_merge_oproj_kernel)
        PGK_REQUIRE(!fused && !direct && group_instantiated(G), "engine: merged o_proj on an unsupported attention path");
        mark(KC_OPROJ);
        a.rows_per_block = e->moproj_rows;
        const dim3 g2((c.hidden_size / e->moproj_rows) * c.num_kv_heads, 1, m);
        PGK_REQUIRE(c.weight_format != 3, "engine: merged o_proj has no NVF4 form");
        const bool f8 = pick.tail == AT_MERGE_OPROJ_FP8;
        he = with_group(G, [&](auto g) {
            constexpr int GG = decltype(g)::value;
            return f8 ? launch_k(attn_merge_oproj_kernel<D, GG, true>, g2, dim3(256), 0, st, a) : launch_k(attn_merge_oproj_kernel<D, GG, false>, g2, dim3(256), 0, st, a);
        });
        PGK_CHECK_HIP(he);
        ++*cx.launches;
    } else if (pick.tail == AT_MERGE) {
        PGK_CHECK_HIP(launch_k(attn_merge_kernel<D>, dim3(c.num_heads, m), dim3(D), 0, st, (const float*)a.part,
                               e->attnv + (size_t)b0 * c.num_heads * D, (int)c.num_heads, (int)a.nsplit));
        ++*cx.launches;
    }
    return PGK_OK;
}

static pgk_status launch_attn(const StepCtx& cx, int layer, const AttnFlags& af) {
    return cx.e->cfg.head_dim == 128 ? launch_attn_d<128>(cx, layer, af) : launch_attn_d<64>(cx, layer, af);
}

}  // namespace pgk
