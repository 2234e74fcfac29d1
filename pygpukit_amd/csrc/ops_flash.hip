// Flash-attention prefill for gfx950 (bf16 / f16, head_dim 64 or 128), second generation: the 16-bit first product and its five
// mask / bias policies.  The orientation (scores transposed, a lane owns a query), the tile walk, V^T staging, the online
// softmax, P.V, the row store and the launch sequence are flash_core.hip.h's, shared with ops_flash_fp8.hip; this file holds
// what forms a tile's scores S^T = K . Q^T on v_mfma_f32_32x32x16 - the K image [64][D], the Q fragments premultiplied by
// scale * log2(e), the start value of the accumulators - and the fp8-output epilogue of the engine's prefill.
// Mask: kv_pos <= (kv_len - q_len) + q_pos  (reference: native/ops/nn/attention_kernels.cuh:32-148).
// The same kernel is Llama-4's sdpa_irope (pgk_sdpa_irope, ops_llama4.hip) when its last argument is a FlashIrope: the
// row's temperature joins the Q premultiply and the mask offset is an argument, kv_pos <= causal_offset + q_pos.
// With a FlashAlibi it is sdpa_alibi (pgk_sdpa_alibi, ops_posenc.hip): the accumulators of S^T start at the ALiBi bias
// -slope[head] * (mask_off + q_pos - kv_pos), in the exp2 domain, instead of at zero - no extra pass over the scores.
// With a FlashFull it is sdpa_noncausal (pgk_sdpa_noncausal, ops_attention.hip): the mask offset is kv_len, so no key is
// ever above a diagonal; q_len may be smaller or larger than kv_len and any q_len >= 1 takes this kernel.
// With a FlashRelBias it is sdpa_relbias (pgk_sdpa_relbias, ops_relbias.hip): FlashFull's mask, and the accumulators of S^T start
// at table[head][clamp(kv_pos - q_pos, -R, R) + R] - the head's row staged once into LDS behind the K / V images.

#include "flash_core.hip.h"

namespace pgk {

// K image: [64 kv][D] 16-bit, 16-byte chunk c (0..D/8-1) of row r at r*2D + ((c ^ (r & (D/8-1))) << 4)
template <int D> __device__ __forceinline__ int fl_k_off(int r, int c) { return r * (2 * D) + ((c ^ (r & (D / 8 - 1))) << 4); }

// X = FlashPlain: sdpa_causal.  X = FlashIrope: sdpa_irope - the two differences are `if constexpr (IROPE)` below.
// X = FlashAlibi: sdpa_alibi - the head's slope and the start value of the score accumulators, `if constexpr (ALIBI)`.
// X = FlashRelBias: sdpa_relbias - FlashFull's mask offset, the staged table row and the start value, `if constexpr (RELBIAS)`.
template <class T, int D, class X = FlashPlain>
__global__ __launch_bounds__(FL_THREADS, 2) void flash_fwd_kernel(const T* q, const T* k, const T* vt, T* out, int hq, int hkv,
                                                              int q_len, int kv_len, int kv_pad, float scale_log2e, FlashStrides sd,
                                                              FlashSplit sp, X ex) {
    constexpr bool IROPE = std::is_same<X, FlashIrope>::value;
    constexpr bool ALIBI = std::is_same<X, FlashAlibi>::value;
    constexpr bool RELBIAS = std::is_same<X, FlashRelBias>::value;
    constexpr bool FULL = std::is_same<X, FlashFull>::value || RELBIAS;
    constexpr int NC = D / 8;            // 16-byte chunks per K row
    constexpr int KS = D / 16;           // k-steps of Q.K^T
    constexpr int DT = D / 32;           // 32-row tiles of O^T
    constexpr int KCH = 64 * NC / FL_THREADS;   // K chunks staged per thread
    constexpr int K_BYTES = 64 * D * 2, V_BYTES = D * 128;
    extern __shared__ __attribute__((aligned(16))) char fl_smem[];   // K[2] | V^T[2]
    auto Ks = [&](int buf) -> char* { return fl_smem + buf * K_BYTES; };

    const int tid = threadIdx.x, lane = tid & 63, ql = lane & 31, h = lane >> 5;
    int mask_off = kv_len - q_len;
    if constexpr (IROPE) mask_off = ex.causal_offset;
    // no diagonal: with the offset at kv_len, kv_end, live() and lim admit every key of every row and only the ragged last
    // tile takes the mask branch (for the keys past kv_len)
    if constexpr (FULL) mask_off = kv_len;
    const FlashWork wk = flash_work(hq, hkv, q_len, sp.nsplit, mask_off);
    const int head = wk.head, qw0 = wk.qw0;
    const T* qh = q + (size_t)head * sd.qh;
    const T* kh = k + (size_t)wk.kvh * sd.kh;

    // Q^T fragments (B operand): lane = query column, k = d
    uint4 qf[KS];
    {
        // Q is pre-multiplied by scale * log2(e) here (one rounding to 16 bits more, inside the 1e-2 bar): the scores come
        // out of the MFMA already in the exp2 domain and the per-tile scaling pass (32 multiplies per lane) disappears
        const T* qrow = qh + (size_t)min(qw0 + ql, q_len - 1) * sd.qs + 8 * h;
        // iRoPE: the row's temperature t(positions[row]) rides in the same multiply - still one rounding to 16 bits
        float qmul = scale_log2e;
        if constexpr (IROPE)
            qmul *= irope_temperature(irope_position(ex.positions, min(qw0 + ql, q_len - 1), ex.pos_is_i64), ex.attn_scale, ex.floor_scale);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            Vec<T> v;
            v.load(qrow + ks * 16);
            float f[8];
            v.to_float(f);
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] *= qmul;
            v.from_float(f);
            qf[ks] = v.raw;
        }
    }
    f32x16_fl o[DT];
#pragma unroll
    for (int i = 0; i < DT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;    // running max (scaled, log2 domain) and this lane's half of the row sum
    // ALiBi: slope * log2(e) of this head (wave-uniform).  The bias of (this lane's query, kv row kv0 + 4h + kvl) is
    // slope2 * (kv0 + 4h + kvl - mask_off - q) <= 0 on every visible key: the integers stay below 2^24 (exact in fp32) and
    // the origin is the same for every tile and KV run of a row, so m_run and the split records need no correction.
    float slope2 = 0.f;
    if constexpr (ALIBI) slope2 = ex.slopes[head] * 1.4426950408889634f;
    // Relative-position bias: entry e of the LDS row is table[head][clamp(e - PAD, 0, 2R)] * log2(e), e in [0, 2R + 1 + 2 PAD).
    // A (wave, tile) pair that is not saturated has kv0 - qw0 in (-R - 64, R + 31), so every index
    // (kv0 + kv_local) - (qw0 + ql) + R + PAD it forms lies in [2, 2R + 2 PAD - 2]: inside the row with no clamp, for rows past
    // q_len and keys past kv_len as well.  rb_lo / rb_hi: the two saturated values (wave-uniform).
    float rb_lo = 0.f, rb_hi = 0.f;
    float* const rb = reinterpret_cast<float*>(fl_smem + 2 * K_BYTES + 2 * V_BYTES);
    int rb_idx = 0;     // + kv0 + local kv row: this lane's entry (negative on its own for late query rows, never once kv0 is added)
    if constexpr (RELBIAS) {
        const int w = 2 * ex.radius + 1;
        const float* trow = ex.table + (size_t)head * w;
        for (int e = tid; e < w + 2 * FL_RELBIAS_PAD; e += FL_THREADS)
            rb[e] = trow[min(max(e - FL_RELBIAS_PAD, 0), w - 1)] * 1.4426950408889634f;    // visible after the barrier below
        rb_lo = trow[0] * 1.4426950408889634f;
        rb_hi = trow[w - 1] * 1.4426950408889634f;
        rb_idx = ex.radius + FL_RELBIAS_PAD + 4 * h - (qw0 + ql);
    }

    // K staging in named registers, as FlashVStage (flash_core.hip.h): chunk i of this thread is c = tid + 256 i, KCH = D / 32 chunks
    static_assert(KCH == DT && (KCH == 2 || KCH == 4), "staging is written for D = 64 / 128");
    uint4 rk0, rk1, rk2, rk3;
    const int kr = tid / NC, kc16 = tid % NC;               // K: row kr + (256/NC) i, chunk kc16
    constexpr int KR_STEP = FL_THREADS / NC;
    FlashVStage<T, DT> vst(tid, kv_pad);
    auto k_src = [&](int kv0, int i) { return kh + (size_t)min(kv0 + kr + KR_STEP * i, kv_len - 1) * sd.ks + kc16 * 8; };
    // Whole tiles address their rows as (wave-uniform tile base) + (per-lane element offset fixed for the kernel): the
    // per-tile address arithmetic is scalar.  (Recomputing min(row, kv_len - 1) * stride per chunk cost 48 vector
    // instructions per tile - 64-bit multiplies included - in a loop that is bound by vector issue.)  Only the ragged
    // last tile clamps its rows.
    const uint32_t ko0 = (uint32_t)(kr * sd.ks + kc16 * 8), ko_step = (uint32_t)(KR_STEP * sd.ks);
    auto load_k = [&](int t) {
        const int kv0 = t * FL_BKV;
        if (kv0 + FL_BKV <= kv_len) {      // wave-uniform
            const T* kt = kh + (size_t)kv0 * sd.ks;
            rk0 = *reinterpret_cast<const uint4*>(kt + ko0);
            rk1 = *reinterpret_cast<const uint4*>(kt + ko0 + ko_step);
            if constexpr (KCH == 4) {
                rk2 = *reinterpret_cast<const uint4*>(kt + ko0 + 2 * ko_step);
                rk3 = *reinterpret_cast<const uint4*>(kt + ko0 + 3 * ko_step);
            }
        } else {
            rk0 = *reinterpret_cast<const uint4*>(k_src(kv0, 0));
            rk1 = *reinterpret_cast<const uint4*>(k_src(kv0, 1));
            if constexpr (KCH == 4) {
                rk2 = *reinterpret_cast<const uint4*>(k_src(kv0, 2));
                rk3 = *reinterpret_cast<const uint4*>(k_src(kv0, 3));
            }
        }
    };
    auto store_k = [&](int buf) {
        char* kb = Ks(buf);
        *reinterpret_cast<uint4*>(kb + fl_k_off<D>(kr, kc16)) = rk0;
        *reinterpret_cast<uint4*>(kb + fl_k_off<D>(kr + KR_STEP, kc16)) = rk1;
        if constexpr (KCH == 4) {
            *reinterpret_cast<uint4*>(kb + fl_k_off<D>(kr + 2 * KR_STEP, kc16)) = rk2;
            *reinterpret_cast<uint4*>(kb + fl_k_off<D>(kr + 3 * KR_STEP, kc16)) = rk3;
        }
    };
    // S^T = K . Q^T of one tile: two 32-kv sub-tiles (rows = positions, column = this lane's query)
    auto qk = [&](int buf, int kv0, f32x16_fl& s0, f32x16_fl& s1) {
        if constexpr (ALIBI) {
            // one FMA per register where the other policies move a zero: literal row offset, per-tile lane base
            const float base = slope2 * (float)(kv0 + 4 * h - (mask_off + qw0 + ql));
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s0[r] = fmaf(slope2, (float)((r & 3) + 8 * (r >> 2)), base);
                s1[r] = fmaf(slope2, (float)(32 + (r & 3) + 8 * (r >> 2)), base);
            }
        } else if constexpr (RELBIAS) {
            const RelbiasTile cls = relbias_tile_class(kv0, qw0, ex.radius);    // wave-uniform
            if (cls == RELBIAS_NEAR) {
                const float* e = rb + (rb_idx + kv0);      // 32 LDS reads at literal offsets from one address
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    s0[r] = e[(r & 3) + 8 * (r >> 2)];
                    s1[r] = e[32 + (r & 3) + 8 * (r >> 2)];
                }
            } else {
                const float b = cls == RELBIAS_FAR_LEFT ? rb_lo : rb_hi;
#pragma unroll
                for (int r = 0; r < 16; ++r) { s0[r] = b; s1[r] = b; }
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) { s0[r] = 0.f; s1[r] = 0.f; }
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const uint4 a0 = *reinterpret_cast<const uint4*>(Ks(buf) + fl_k_off<D>(ql, 2 * ks + h));
            const uint4 a1 = *reinterpret_cast<const uint4*>(Ks(buf) + fl_k_off<D>(32 + ql, 2 * ks + h));
            s0 = mfma32<T>(a0, qf[ks], s0);
            s1 = mfma32<T>(a1, qf[ks], s1);
        }
    };
    auto retire_q = [&] {      // why: flash_walk
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) asm volatile("" ::"v"(qf[ks].x), "v"(qf[ks].y), "v"(qf[ks].z), "v"(qf[ks].w));
    };
    flash_walk<T, DT, false>(wk, vst, vt + (size_t)wk.kvh * D * kv_pad, q_len, kv_len, sp.nsplit, ql, h, fl_smem + 2 * K_BYTES, o, m_run, l_run, 1.0f, load_k,
                             store_k, retire_q, qk);

    float inv;
    const float l_tot = flash_row_sum(l_run, inv);
    if constexpr (std::is_same<T, bf16>::value && D == 128 && std::is_same<X, FlashPlain>::value) {
        if (sp.q8 != nullptr && sp.nsplit == 1) {       // workgroup-uniform
            // the lane's 64 dims (the partner lane ^ 32 holds the other 64), rounded to bf16 as the plain store would
            float amax = 0.f;
#pragma unroll
            for (int i = 0; i < DT; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    o[i][e] = __uint_as_float(pack_bf16x2(o[i][e] * inv, 0.f) << 16);
                    amax = fmaxf(amax, fabsf(o[i][e]));
                }
            amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
            const float sc = amax > 0.f ? amax / 448.0f : 1.0f;
            const int qrow = qw0 + ql;
            if (qrow < q_len) {
                uint8_t* qrow8 = sp.q8 + ((size_t)qrow * hq + head) * D;
#pragma unroll
                for (int i = 0; i < DT; ++i)
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        *reinterpret_cast<uint32_t*>(qrow8 + i * 32 + 8 * g + 4 * h) =
                            pack_fp8x4(o[i][4 * g] / sc, o[i][4 * g + 1] / sc, o[i][4 * g + 2] / sc, o[i][4 * g + 3] / sc);
                if (h == 0) sp.q8s[(size_t)qrow * hq + head] = sc;
            }
            return;
        }
    }
    flash_store_row<T, DT>(wk, o, m_run, l_tot, inv, ql, h, out, hq, q_len, sd, sp);
}

// kv_seen: the keys the heaviest query tile walks (sdpa_causal: all of them; sdpa_irope: min(kv_len, causal_offset + q_len))
template <class T, int D, class X = FlashPlain>
static pgk_status flash_launch(const T* q, const T* k, const T* v, T* out, int hq, int hkv, int q_len, int kv_len, float scale,
                               const FlashStrides& sd, hipStream_t st, uint8_t* q8 = nullptr, float* q8s = nullptr, X ex = X{},
                               int kv_seen = 0) {
    // FlashRelBias: the table row sits behind the K / V images; the attribute is set once for the largest row
    size_t lds_extra = 0, lds_extra_max = 0;
    if constexpr (std::is_same<X, FlashRelBias>::value) {
        lds_extra = relbias_lds_bytes(ex.radius);
        lds_extra_max = relbias_lds_bytes(FL_RELBIAS_MAX_RADIUS);
    }
    const FlashPlan p = flash_plan(hq, hkv, q_len, kv_len, kv_seen > 0 ? kv_seen : kv_len, D, device_cu_count());
    constexpr size_t LDS = 2 * (size_t)(64 * D * 2) + 2 * (size_t)(D * 128);
    static bool attr_done = false;
    if (LDS + lds_extra_max > 48 * 1024 && !attr_done) {
        PGK_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&flash_fwd_kernel<T, D, X>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)(LDS + lds_extra_max)));
        attr_done = true;
    }
    void* ws = nullptr;
    if (pgk_status r = pgk_malloc(&ws, p.bytes)) return r;
    const FlashSplit sp = flash_split(p, ws, q8, q8s);
    const hipError_t e = flash_run<T, D>(p, ws, sp, v, out, hq, hkv, q_len, kv_len, sd, st, [&](int grid, const T* vt) {
        flash_fwd_kernel<T, D, X><<<grid, FL_THREADS, LDS + lds_extra, st>>>(q, k, vt, out, hq, hkv, q_len, kv_len, p.kv_pad,
                                                                            scale * 1.4426950408889634f, sd, sp, ex);
    });
    pgk_free(ws);   // stream-ordered reuse: later work on this stream runs after the kernels above
    PGK_CHECK_HIP(e);
    return PGK_OK;
}

// (dt16, d) -> flash_launch<T, D, X> for any policy; dt16: 0 = bf16, 1 = f16, d: 64 or 128
template <class X>
static pgk_status flash_launch_any(int dt16, int d, const void* q, const void* k, const void* v, void* out, int hq, int hkv, int q_len,
                                   int kv_len, float scale, const FlashStrides& sd, hipStream_t st, X ex, int kv_seen) {
    auto run = [&](auto* t, auto dd) {
        using T = std::remove_pointer_t<decltype(t)>;
        return flash_launch<T, decltype(dd)::value, X>((const T*)q, (const T*)k, (const T*)v, (T*)out, hq, hkv, q_len, kv_len, scale, sd, st,
                                                       nullptr, nullptr, ex, kv_seen);
    };
    const std::integral_constant<int, 128> d128;
    const std::integral_constant<int, 64> d64;
    if (dt16 == 0) return d == 128 ? run((bf16*)nullptr, d128) : run((bf16*)nullptr, d64);
    return d == 128 ? run((f16*)nullptr, d128) : run((f16*)nullptr, d64);
}

// The entries of attn_plan.h; their callers (ops_attention.hip, ops_llama4.hip, ops_posenc.hip) have checked the arguments.
pgk_status flash_prefill(const void* q, const void* k, const void* v, void* out, int hq, int hkv, int q_len, int kv_len, int d, float scale,
                         const FlashStrides& sd, int dt16, hipStream_t st) {
    return flash_launch_any(dt16, d, q, k, v, out, hq, hkv, q_len, kv_len, scale, sd, st, FlashPlain{}, 0);
}

// every KV run of every query tile is live, so the split heuristic sees all kv_len keys
pgk_status flash_prefill_full(const void* q, const void* k, const void* v, void* out, int hq, int hkv, int q_len, int kv_len, int d,
                              float scale, const FlashStrides& sd, int dt16, hipStream_t st) {
    return flash_launch_any(dt16, d, q, k, v, out, hq, hkv, q_len, kv_len, scale, sd, st, FlashFull{}, kv_len);
}

// scale is 1/sqrt(d); row i sees kv j <= i + causal_offset (>= 0), so an offset beyond kv_len masks nothing and is clamped to it
pgk_status flash_prefill_irope(const void* q, const void* k, const void* v, const void* positions, void* out, int hq, int hkv, int q_len,
                               int kv_len, int d, float attn_scale, float floor_scale, int causal_offset, const FlashStrides& sd,
                               int pos_is_i64, int dt16, hipStream_t st) {
    const int off = causal_offset < kv_len ? causal_offset : kv_len;
    const FlashIrope ex{positions, attn_scale, floor_scale, off, pos_is_i64};
    const int kv_seen = (long long)off + q_len < kv_len ? off + q_len : kv_len;
    return flash_launch_any(dt16, d, q, k, v, out, hq, hkv, q_len, kv_len, 1.0f / sqrtf((float)d), sd, st, ex, kv_seen);
}

// scale > 0, kv_len >= q_len; slopes: [hq] fp32 on the device
pgk_status flash_prefill_alibi(const void* q, const void* k, const void* v, const float* slopes, void* out, int hq, int hkv, int q_len,
                               int kv_len, int d, float scale, const FlashStrides& sd, int dt16, hipStream_t st) {
    return flash_launch_any(dt16, d, q, k, v, out, hq, hkv, q_len, kv_len, scale, sd, st, FlashAlibi{slopes}, 0);
}

// every KV run of every query tile is live, as in flash_prefill_full; the callers have checked 0 <= radius <= FL_RELBIAS_MAX_RADIUS
pgk_status flash_prefill_relbias(const void* q, const void* k, const void* v, const float* table, void* out, int hq, int hkv, int q_len,
                                 int kv_len, int d, int radius, float scale, const FlashStrides& sd, int dt16, hipStream_t st) {
    return flash_launch_any(dt16, d, q, k, v, out, hq, hkv, q_len, kv_len, scale, sd, st, FlashRelBias{table, radius}, kv_len);
}

// engine entry (fp8 x fp8 prefill, bf16, head_dim 128, q_len > 128): causal attention whose result leaves as the o_proj's fp8
// operand - codes [q_len][hq * 128] + scales [q_len][hq] - instead of bf16 rows (FlashSplit::q8)
pgk_status flash_prefill_q8(const void* q, const void* k, const void* v, uint8_t* q8, float* q8s, int hq, int hkv, int q_len, int kv_len,
                            float scale, long long qh, long long qs, long long kh, long long ks, hipStream_t st) {
    PGK_REQUIRE(q8 && q8s && q_len > 128, "flash_prefill_q8: needs output buffers and q_len > 128 (got %d)", q_len);
    const FlashStrides sd{qh, qs, kh, ks, 0, 0};
    return flash_launch<bf16, 128>((const bf16*)q, (const bf16*)k, (const bf16*)v, nullptr, hq, hkv, q_len, kv_len, scale, sd, st, q8, q8s);
}

}  // namespace pgk
