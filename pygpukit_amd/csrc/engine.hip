// Native decode / prefill engine for Qwen3 / Llama-shaped causal transformers on gfx950.
//
// A decode step is a short chain of fused weight-streaming kernels, enqueued by ONE C call and captured
// into ONE hipGraph whose per-sequence token id and position live in device memory:
//
//   per layer (fused path, contexts <= 512):
//     norm_qkv          qkv[b]      = Wqkv . rmsnorm(h[b])
//     attn_oproj        part[b][kv] = Wo[:, heads of kv] . attention(q,k,v of kv head)   (QK-norm, RoPE, KV write inside)
//     norm_gateup       h2[b] = h[b] + sum_kv part[b][kv] ;  act[b] = silu(Wg x) * (Wu x),  x = rmsnorm(h2[b])
//     down_residual     h[b]  = h2[b] + Wd . act[b]
//   per layer (split path, long contexts): norm_qkv, split-KV attn, oproj_residual, norm_gateup, down_residual
//   norm_lmhead         logits[b]   = E . rmsnorm(h[b])  (+ per-workgroup argmax partials)
//   finalize            token[b] = argmax (lowest index on ties); position[b] += 1; log; h[b] = E[token[b]]
//
// i.e. 4L+2 launches per token versus ~21 launches + 21 device syncs per layer in the reference's eager
// step and 2L+2 graphs in its "graph" step (src/pygpukit/llm/decode/m1.py:40-121,
// m1_graph.py:463-589).  On this chip a dependent kernel boundary (~1.7 us in a graph) is the cheapest
// chip-wide synchronisation there is, so the design minimises the NUMBER of boundaries and, inside each
// kernel, issues the weight loads BEFORE the activation prologue so the two memory round trips overlap.
// The residual stream, q/k/v and the MLP activation stay fp32 between kernels; only the KV cache (bf16)
// and the weights are rounded.  KV cache layout: [layer][seq][Hkv][max_seq][D] - un-expanded GQA.
//
// Prefill runs the MFMA GEMM / flash-attention kernels on bf16 activations with an fp32 residual stream.
// (engine_prefill.hip; this file: the decode step, create / destroy, capture / replay, probes.  File map: DESIGN.md 1.)

#include "engine_attn.hip.h"
#include "engine_gemv.hip.h"
#include "pkgemm.hip.h"

namespace pgk {

// h[b][:] = E[token[b]][:]   (step entry: pgk_engine_set_state; afterwards finalize_kernel keeps h current)
__global__ void embed_kernel(const bf16* embed, const int32_t* tokens, float* h, int H, const int32_t* positions,
                             const float* rope_cos, const float* rope_sin, float* cur_cos, float* cur_sin, int half,
                             int max_seq) {
    const int b = blockIdx.x;
    const bf16* row = embed + (size_t)tokens[b] * H;
    for (int i = threadIdx.x; i < H; i += blockDim.x) h[(size_t)b * H + i] = to_f(row[i]);
    const int pos = min(positions[b], max_seq - 1);
    for (int i = threadIdx.x; i < half; i += blockDim.x) {
        cur_cos[(size_t)b * half + i] = rope_cos[(size_t)pos * half + i];
        cur_sin[(size_t)b * half + i] = rope_sin[(size_t)pos * half + i];
    }
}

// token[b] = argmax over workgroup partials (ties -> lowest index); position[b] += 1; log the token;
// h[b] = E[token] for the next step; the last workgroup of the step's last chunk bumps the step counter.
// One workgroup per sequence (grid = M).  Every workgroup reads the step counter before it takes an arrival ticket
// (step_counter[1]); the bump is made by whoever draws the last ticket, so it cannot overtake a read.  (One workgroup
// for the whole chunk, a wave per sequence, took 25 us at M = 8 and 57 us at M = 16 - a dependent walk per sequence.)
__global__ __launch_bounds__(256) void finalize_kernel(unsigned long long* tl, const float* amax_val, const int* amax_idx, int nblk,
                                                       int32_t* tokens, int32_t* positions, int32_t* token_log,
                                                       int32_t* step_counter, int log_width, int log_cap,
                                                       const bf16* embed, float* h, int H, int bump,
                                                       unsigned long long* clk_log, const float* rope_cos,
                                                       const float* rope_sin, float* cur_cos, float* cur_sin, int half,
                                                       int max_seq, int M, const int32_t* sampled) {
    const TLStamp tls(tl);
    __shared__ float sv[4];
    __shared__ int si[4];
    __shared__ int s_tok, s_pos;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, b = blockIdx.x;
    const int step = step_counter[0];
    int bi;
    if (sampled) {
        bi = sampled[b];                                  // temperature / top-k / top-p draw (ops_sampling.hip)
    } else {
        float bv = -INFINITY;
        bi = 0x7FFFFFFF;
        for (int i = threadIdx.x; i < nblk; i += 256) {
            const float v = amax_val[(size_t)b * nblk + i];
            const int ix = amax_idx[(size_t)b * nblk + i];
            if (v > bv || (v == bv && ix < bi)) { bv = v; bi = ix; }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float ov = __shfl_xor(bv, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { sv[wid] = bv; si[wid] = bi; }
        __syncthreads();
        bv = sv[0]; bi = si[0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (sv[w] > bv || (sv[w] == bv && si[w] < bi)) { bv = sv[w]; bi = si[w]; }
        if (bi == 0x7FFFFFFF) bi = 0;
    }
    if (threadIdx.x == 0) {
        s_tok = bi;
        tokens[b] = bi;
        const int npos = positions[b] + 1;
        positions[b] = npos;
        s_pos = min(npos, max_seq - 1);
        if (step < log_cap) token_log[(size_t)step * log_width + b] = bi;
        if (b == 0 && step < log_cap && clk_log) {  // shader-clock / 100 MHz wall-clock stamps (diagnostic only)
            clk_log[2 * (size_t)step] = __builtin_amdgcn_s_memtime();
            clk_log[2 * (size_t)step + 1] = __builtin_amdgcn_s_memrealtime();
        }
    }
    __syncthreads();
    // next step's inputs of this sequence: its embedding row (8 bf16 per lane) and the RoPE row of its next position
    const bf16* erow = embed + (size_t)s_tok * H;
    float* hrow = h + (size_t)b * H;
    if ((H & 7) == 0) {
        for (int v = threadIdx.x; v < (H >> 3); v += 256) {
            const uint4 raw = *reinterpret_cast<const uint4*>(erow + v * 8);
            float f[8];
            WTraits<bf16>::decode(raw, f);
            *reinterpret_cast<float4*>(hrow + v * 8) = make_float4(f[0], f[1], f[2], f[3]);
            *reinterpret_cast<float4*>(hrow + v * 8 + 4) = make_float4(f[4], f[5], f[6], f[7]);
        }
    } else {
        for (int i = threadIdx.x; i < H; i += 256) hrow[i] = to_f(erow[i]);
    }
    for (int i = threadIdx.x; i < half; i += 256) {
        cur_cos[(size_t)b * half + i] = rope_cos[(size_t)s_pos * half + i];
        cur_sin[(size_t)b * half + i] = rope_sin[(size_t)s_pos * half + i];
    }
    if (bump && threadIdx.x == 0) {
        if (M == 1) {
            step_counter[0] = step + 1;
        } else if (atomicAdd(&step_counter[1], 1) == M - 1) {   // every workgroup has read `step` before its own ticket
            atomicExch(&step_counter[1], 0);
            step_counter[0] = step + 1;
        }
    }
    tls.end();
}

thread_local Probe* g_probe = nullptr;   // measurement hooks: engine_common.hip.h

pgk_status sample_rows_ring(const float* logits, int rows, int vocab, float temperature, int top_k, float top_p, const float* u_ring,
                            int u_cap, int u_stride, const int32_t* step_counter, int32_t* out, void* scratch, hipStream_t st);
size_t sample_scratch_bytes(int rows, int vocab, int top_k, float top_p);

// The four projections of a layer for the chunk of sequences that starts at b0: weights, shape and the fp32 buffers every
// path uses.  A caller adds only what is its own: xin16 / wp / out16, part / nsplit / h_out, another residual.
// out[b] = W . rmsnorm(h[b]) * gamma, N outputs per sequence
static FusedArgs norm_proj_args(const Engine* e, int b0, const void* w, const void* s, const void* gamma, int N, float* out) {
    const int H = e->cfg.hidden_size;
    FusedArgs a{};
    a.w = w; a.wscale = (const bf16*)s; a.N = N; a.K = H;
    a.h = e->h + (size_t)b0 * H; a.gamma = (const bf16*)gamma; a.eps = e->cfg.norm_eps;
    a.out = out + (size_t)b0 * N; a.ld_out = N;
    return a;
}
// h[b] += W . xin[b], K inputs per sequence
static FusedArgs resid_proj_args(const Engine* e, int b0, const void* w, const void* s, int K, const float* xin) {
    const int H = e->cfg.hidden_size;
    FusedArgs a{};
    a.w = w; a.wscale = (const bf16*)s; a.N = H; a.K = K;
    a.xin = xin + (size_t)b0 * K;
    a.res = e->h + (size_t)b0 * H; a.out = e->h + (size_t)b0 * H; a.ld_out = H;
    return a;
}
static FusedArgs qkv_args(const Engine* e, const pgk_layer_weights_t& L, int b0) { return norm_proj_args(e, b0, L.w_qkv, L.s_qkv, L.attn_norm, e->qkv_dim(), e->qkv); }
static FusedArgs o_args(const Engine* e, const pgk_layer_weights_t& L, int b0) { return resid_proj_args(e, b0, L.w_o, L.s_o, e->cfg.num_heads * e->cfg.head_dim, e->attnv); }
static FusedArgs gate_up_args(const Engine* e, const pgk_layer_weights_t& L, int b0) { return norm_proj_args(e, b0, L.w_gate_up, L.s_gate_up, L.mlp_norm, e->cfg.intermediate_size, e->act); }
static FusedArgs down_args(const Engine* e, const pgk_layer_weights_t& L, int b0) { return resid_proj_args(e, b0, L.w_down, L.s_down, e->cfg.intermediate_size, e->act); }

// The tail of every chunk: logits = E . rmsnorm(h) (lm_head stays bf16 even when the linears are fp8) with `nblk` argmax
// partials per sequence, `stride` slots apart; the optional draw; finalize.  `lm_head(a)` adds what its kernels read
// besides (xin16, wp) and launches them.  `last` = this is the step's last chunk (bumps the step counter).
template <class LmHead>
static pgk_status finish_chunk(const StepCtx& cx, bool last, int nblk, int stride, LmHead lm_head) {
    Engine* e = cx.e;
    const auto& c = e->cfg;
    const int H = c.hidden_size, D = c.head_dim, b0 = cx.b0, M = cx.M;
    float* h = e->h + (size_t)b0 * H;
    mark(KC_LMHEAD);
    FusedArgs a = norm_proj_args(e, b0, e->lm_head, nullptr, e->final_norm, c.vocab_size, e->logits);
    a.amax_val = e->amax_val + (size_t)b0 * stride; a.amax_idx = e->amax_idx + (size_t)b0 * stride;
    if (pgk_status r = counted(cx.launches, lm_head(a))) return r;
    mark(KC_ARGMAX);
    const int32_t* sampled = nullptr;
    if (e->sample_temperature > 0.f) {
        // one draw per sequence of the chunk from the fp32 logits the lm_head kernel just wrote; the uniform numbers come from
        // the device ring row (step counter % u_cap), so a captured graph replays with fresh randomness the host queued up
        if (pgk_status r = counted(cx.launches, sample_rows_ring(a.out, M, c.vocab_size, e->sample_temperature, e->sample_top_k, e->sample_top_p, e->u_ring + b0,
                                                                 e->u_cap, c.max_batch, e->step_counter, e->sampled + b0, e->sample_scratch, cx.st))) return r;
        sampled = e->sampled + b0;
    }
    PGK_CHECK_HIP(launch_k(finalize_kernel, dim3(M), dim3(256), 0, cx.st, a.amax_val, a.amax_idx, nblk, e->tokens + b0, e->positions + b0, e->token_log + b0, e->step_counter,
                                       e->cfg.max_batch, e->log_cap, e->embed, h, H, last ? 1 : 0, b0 == 0 ? e->clk_log : nullptr,
                                       e->rope_cos, e->rope_sin, e->cur_cos + (size_t)b0 * (D / 2), e->cur_sin + (size_t)b0 * (D / 2),
                                       D / 2, c.max_seq_len, M, sampled));
    ++*cx.launches;
    return PGK_OK;
}

// One decode step for sequences [b0, b0+M); `last` = this is the step's last chunk (bumps the step counter).
// `short_ctx`: every sequence of the step has at most SHORT_CTX positions - a single sequence then takes the fused
// attention + o_proj kernel (4 L + 2 launches); otherwise split-KV slices + merge/o_proj (5 L + 2).  Both are correct at
// any context: the choice follows the context of the step, not the capacity of the cache (pgk_engine_replay).
template <class WT, class XT, int M>
static pgk_status decode_chunk(const StepCtx& cx, bool last) {
    Engine* e = cx.e;
    const auto& c = e->cfg;
    const int H = c.hidden_size, I = c.intermediate_size, b0 = cx.b0;
    const hipStream_t st = cx.st;
    float* h = e->h + (size_t)b0 * H;
    float* h2 = e->h2 + (size_t)b0 * H;
    const AttnFlags af = attn_flags(e, CF_GEMV, M, cx.short_ctx);   // engine_state.hip.h
    const bool fused = af.fused, direct = af.direct, merged = af.merged;
    const bool partials = fused || merged;
    for (int l = 0; l < c.num_layers; ++l) {
        const auto& L = e->layers[l];
        // 1. qkv = Wqkv . rmsnorm(h)
        mark(KC_NORM_QKV);
        FusedArgs a = qkv_args(e, L, b0);
        if (pgk_status r = counted(cx.launches, launch_fused_auto<WT, XT, M, PRO_NORM, EPI_STORE>(a, a.N, st))) return r;
        mark(KC_ATTN);
        // 2. attention (QK-norm, RoPE, KV write fused; on the fused path also the o_proj partial products)
        if (pgk_status r = launch_attn(cx, l, af)) return r;
        const float* mlp_in = h;
        if (!partials) {
            mark(KC_OPROJ);
            // 3. h += Wo . attn   (attn = merged split-KV records, written by attn_merge_kernel)
            a = o_args(e, L, b0);
            if (pgk_status r = counted(cx.launches, launch_fused_auto<WT, XT, M, PRO_PLAIN, EPI_RESID>(a, H, st))) return r;
        }
        // 4. act = silu(Wg x) * (Wu x), x = rmsnorm(h [+ sum of o_proj partials])
        mark(KC_GATEUP);
        a = gate_up_args(e, L, b0);
        pgk_status gr;
        if constexpr (M <= 2) {   // per-kv-head o_proj partials only ever exist for one or two sequences per chunk
            if (partials) { a.part = e->opart + (size_t)b0 * c.num_kv_heads * H; a.nsplit = c.num_kv_heads; a.h_out = h2; mlp_in = h2; }
            gr = partials ? launch_fused_auto<WT, XT, M, PRO_NORM_SUM, EPI_SWIGLU>(a, I, st) : launch_fused_auto<WT, XT, M, PRO_NORM, EPI_SWIGLU>(a, I, st);
        } else gr = launch_fused_auto<WT, XT, M, PRO_NORM, EPI_SWIGLU>(a, I, st);
        if (pgk_status r = counted(cx.launches, gr)) return r;
        // 5. h = mlp_in + Wd . act
        mark(KC_DOWN);
        a = down_args(e, L, b0);
        a.res = mlp_in;
        if (pgk_status r = counted(cx.launches, launch_fused_auto<WT, XT, M, PRO_PLAIN, EPI_RESID>(a, H, st))) return r;
    }
    return finish_chunk(cx, last, e->lm_blocks, e->lm_blocks, [&](FusedArgs& a) {
        return launch_fused<bf16, XT, M, 4, PRO_NORM, EPI_LOGITS>(a, c.vocab_size, st, e->lm_blocks);
    });
}

// 3..64 sequences per chunk: every projection on the MFMA kernels of engine_batched.hip.  Up to 16 sequences the cost of
// a projection does not depend on M and RMSNorm is fused into the consumer's prologue (5 L + 2 launches at short
// context); 17..64 sequences run the M-tiled kernels - each weight byte is still read ONCE per step - on rows that one
// small launch per norm has already normalised to bf16 (7 L + 3 launches).  Attention is per sequence either way.
template <class WT>
static pgk_status decode_chunk_batched(const StepCtx& cx, bool last) {
    Engine* e = cx.e;
    const auto& c = e->cfg;
    constexpr bool FP8 = std::is_same<WT, fp8e4m3>::value;
    const int H = c.hidden_size, I = c.intermediate_size, QD = c.num_heads * c.head_dim, b0 = cx.b0, M = cx.M;
    const hipStream_t st = cx.st;
    float* h = e->h + (size_t)b0 * H;
    bf16* x16 = e->x16 + (size_t)b0 * H;
    const bool tiled = M > 16;
    const AttnFlags af = attn_flags(e, tiled ? CF_TILED : CF_BATCHED, M, cx.short_ctx);
    const bool direct = af.direct;
    // tiled: the consumer reads rows that a launch of their own has normalised to bf16
    auto norm_x16 = [&](FusedArgs& a) -> pgk_status {
        if (!tiled) return PGK_OK;
        a.xin16 = x16;
        return counted(cx.launches, norm_rows_bf16(h, a.gamma, x16, M, H, c.norm_eps, st));
    };
    for (int l = 0; l < c.num_layers; ++l) {
        const auto& L = e->layers[l];
        mark(KC_NORM_QKV);
        FusedArgs a = qkv_args(e, L, b0);
        if (pgk_status r = norm_x16(a)) return r;
        // 16-row workgroups (N / 16 >= 192) stream the fragment-major copy where the engine holds one: one coalesced KiB per
        // load instead of 64 separate 16-byte pieces of the row-major matrix (the batched lm_head's gain)
        if (batched_layer_copy(e, FP8)) a.wp = e->packed[l].qkv;
        if (pgk_status r = counted(cx.launches, batched_proj(FP8, tiled ? PRO_PLAIN : PRO_NORM, EPI_STORE, a, M, st))) return r;
        mark(KC_ATTN);
        if (pgk_status r = launch_attn(cx, l, af)) return r;
        mark(KC_OPROJ);
        a = o_args(e, L, b0);
        if (direct || tiled) a.xin16 = e->attnv16 + (size_t)b0 * QD;   // the whole-context attention kernel wrote bf16
        if (tiled && !direct) {   // long contexts: the merge kernel leaves fp32 rows; the tiled kernels read bf16 fragments
            if (pgk_status r = counted(cx.launches, norm_rows_bf16(a.xin, nullptr, e->attnv16 + (size_t)b0 * QD, M, QD, 0.f, st))) return r;
        }
        if (pgk_status r = counted(cx.launches, batched_proj(FP8, PRO_PLAIN, EPI_RESID, a, M, st))) return r;
        mark(KC_GATEUP);
        a = gate_up_args(e, L, b0);
        a.out16 = e->act16 + (size_t)b0 * I;        // SiLU(g) * u leaves as bf16: down_proj rounds it to bf16 anyway
        if (pgk_status r = norm_x16(a)) return r;
        if (batched_layer_copy(e, FP8)) a.wp = e->packed[l].gate_up;
        if (pgk_status r = counted(cx.launches, batched_proj(FP8, tiled ? PRO_PLAIN : PRO_NORM, EPI_SWIGLU, a, M, st))) return r;
        mark(KC_DOWN);
        a = down_args(e, L, b0);
        a.xin16 = e->act16 + (size_t)b0 * I;
        if (pgk_status r = counted(cx.launches, batched_proj(FP8, PRO_PLAIN, EPI_RESID, a, M, st))) return r;
    }
    const int nblk = batched_lm_blocks(c.vocab_size);   // engine_state.hip.h
    return finish_chunk(cx, last, nblk, e->lm_cap, [&](FusedArgs& a) -> pgk_status {
        a.wp = e->packed_lm;
        // the final norm keeps its launch: 2048 lm_head workgroups re-deriving the row statistic would read 128 MB of partials
        if (pgk_status r = norm_x16(a)) return r;
        return batched_proj(false, tiled ? PRO_PLAIN : PRO_NORM, EPI_LOGITS, a, M, st, nblk);
    });
}

// 17..64 sequences, bf16 layers: the step on the fragment-major weight copy (ops_pkgemm.hip) - the prefill's kernels with
// one row per SEQUENCE.  Seven launches per layer as on the tiled path, but the projections stream coalesced 1 KiB
// fragments with the activation block in LDS by DMA, SwiGLU sits in the gate_up epilogue, and the N = hidden projections
// are split along K over 256 workgroups with the next RMSNorm summing their slabs (rmsnorm_f32_bf16_kernel, as in
// pgk_engine_prefill).  Attention (per-sequence positions, new-token norm / RoPE / cache write) is the batch kernel.
static pgk_status decode_chunk_packed(const StepCtx& cx, bool last) {
    Engine* e = cx.e;
    const auto& c = e->cfg;
    const int H = c.hidden_size, I = c.intermediate_size, QD = c.num_heads * c.head_dim, NQKV = e->qkv_dim(), b0 = cx.b0, M = cx.M;
    const hipStream_t st = cx.st;
    float* h = e->h + (size_t)b0 * H;
    bf16* x16 = e->x16 + (size_t)b0 * H;
    const AttnFlags af = attn_flags(e, CF_PACKED, M, cx.short_ctx);
    const bool direct = af.direct;
    const int s_o = pkgemm_pick_splits(M, H, QD), s_d = pkgemm_pick_splits(M, H, I);
    int pending = 0;
    auto norm = [&](const bf16* gamma) -> pgk_status {
        mark(KC_NORM_QKV);
        // (plain launches, like the projections of this path: the per-launch probe and the in-kernel timeline cover the
        // kernels that take a timeline pointer - attention, lm_head, finalize)
        return rmsnorm_slabs(h, gamma, x16, M, H, c.norm_eps, e->dec_slabs, &pending, nullptr, nullptr, st, cx.launches);
    };
    const bool carried = e->packed_resid;      // o_proj / down_proj carry the next RMSNorm: 5 launches per layer instead of 7
    int ss_n = 0;
    for (int l = 0; l < c.num_layers; ++l) {
        const auto& L = e->layers[l];
        const auto& P = e->packed[l];
        PkArgs nrm{};
        if (carried && l > 0) { nrm.ss_in = e->pk_ss; nrm.ss_n = ss_n; nrm.ss_eps = c.norm_eps; }
        else if (pgk_status r = norm((const bf16*)L.attn_norm)) return r;
        if (pgk_status r = counted(cx.launches, pkgemm_nt(x16, H, P.qkv, e->qkv + (size_t)b0 * NQKV, NQKV, PK_EPI_SLAB, 1, M, NQKV, H, &nrm, st))) return r;
        mark(KC_ATTN);
        if (pgk_status r = launch_attn(cx, l, af)) return r;
        mark(KC_OPROJ);
        bf16* attn16 = e->attnv16 + (size_t)b0 * QD;
        if (!direct) {   // long contexts: the merge kernel leaves fp32 rows
            if (pgk_status r = counted(cx.launches, norm_rows_bf16(e->attnv + (size_t)b0 * QD, nullptr, attn16, M, QD, 0.f, st))) return r;
        }
        bf16* act16 = e->act16 + (size_t)b0 * I;
        if (carried) {
            if (pgk_status r = packed_mlp_carried(e, l, M, attn16, act16, h, x16, &ss_n, st, cx.launches)) return r;
            continue;
        }
        if (pgk_status r = counted(cx.launches, pkgemm_nt(attn16, QD, P.o, e->dec_slabs, H, PK_EPI_SLAB, s_o, M, H, QD, nullptr, st))) return r;
        pending = s_o;
        if (pgk_status r = norm((const bf16*)L.mlp_norm)) return r;
        mark(KC_GATEUP);
        if (pgk_status r = counted(cx.launches, pkgemm_nt(x16, H, P.gate_up, act16, I, PK_EPI_SWIGLU, 1, M, 2 * I, H, nullptr, st))) return r;
        mark(KC_DOWN);
        if (pgk_status r = counted(cx.launches, pkgemm_nt(act16, I, P.down, e->dec_slabs, H, PK_EPI_SLAB, s_d, M, H, I, nullptr, st))) return r;
        pending = s_d;
    }
    const int nblk = batched_lm_blocks(c.vocab_size);   // engine_state.hip.h
    if (pgk_status r = norm(e->final_norm)) return r;     // also folds the last down_proj's slabs into the residual stream
    return finish_chunk(cx, last, nblk, e->lm_cap, [&](FusedArgs& a) {
        a.xin16 = x16;
        a.wp = e->packed_lm;                                  // the M-tiled lm_head streams the fragment-major copy too
        // (lm_head on a packed copy with an argmax epilogue was built and measured: 1.342 ms per step against 1.331 at 64
        // sequences - its 39 MB of fp32 logits stores, not the weight loads, are what the row-major kernel's 95 us are made of)
        return batched_proj(false, PRO_PLAIN, EPI_LOGITS, a, M, st, nblk);
    });
}

template <class WT>
static pgk_status decode_step_impl(Engine* e, int batch, hipStream_t st, int* launches, bool short_ctx) {
    int b0 = 0;
    while (b0 < batch) {
        const int rem = batch - b0;
        auto chunk = [&](int m) { return StepCtx{e, b0, m, st, launches, short_ctx}; };
        pgk_status r;
        const ChunkChoice ch = next_chunk(e, rem);   // engine_state.hip.h
        const int m = ch.m;
        if constexpr (std::is_same<WT, nvf4x2>::value) {
            // NVF4 (w4a16): GEMV chunks only (next_chunk); the MFMA chunk kernels are not instantiated for it
        } else if (ch.form != CF_GEMV) {
            if (ch.form == CF_PACKED) r = decode_chunk_packed(chunk(m), rem == m);
            else r = decode_chunk_batched<WT>(chunk(m), rem == m);
            b0 += m;
            if (r != PGK_OK) return r;
            continue;
        }
        if (m == 8) r = decode_chunk<WT, bf16, 8>(chunk(8), rem == 8);
        else if (m == 4) r = decode_chunk<WT, bf16, 4>(chunk(4), rem == 4);
        else if (m == 2) r = decode_chunk<WT, float, 2>(chunk(2), rem == 2);
        else r = decode_chunk<WT, float, 1>(chunk(1), true);
        b0 += m;
        if (r != PGK_OK) return r;
    }
    return PGK_OK;
}

// short_ctx: the step's launch sequence for contexts <= SHORT_CTX (ignored - long sequence - when the engine has no such path)
static pgk_status decode_step(Engine* e, int batch, hipStream_t st, int* launches, bool short_ctx) {
    short_ctx = short_ctx && e->short_path;
    if (e->cfg.weight_format == 3) return decode_step_impl<nvf4x2>(e, batch, st, launches, short_ctx);
    if (e->cfg.weight_format != 0) return decode_step_impl<fp8e4m3>(e, batch, st, launches, short_ctx);
    return decode_step_impl<bf16>(e, batch, st, launches, short_ctx);
}

// One step enqueued (eagerly or into a capture) at the host-side position bound: its split-KV slicing and launch sequence, then
// the bound moves on by `advance`.  *launches (optional): the step's launch count; probe (optional): installed for the step.
static pgk_status enqueue_step(Engine* e, int batch, hipStream_t st, int advance, int* launches = nullptr, Probe* probe = nullptr) {
    int n = 0;
    e->step_span = span_for(e);
    g_probe = probe;
    const pgk_status r = decode_step(e, batch, st, &n, step_is_short(e, batch));
    g_probe = nullptr;
    if (launches) *launches = n;
    if (e->pos_hi >= 0) e->pos_hi += advance;
    return r;
}

static void drop_graphs(Engine* e) {
    for (auto& t : e->tiers) {
        if (t.exec) (void)hipGraphExecDestroy(t.exec);
        if (t.graph) (void)hipGraphDestroy(t.graph);
    }
    e->tiers.clear();
    e->graph_batch = 0;
}

}  // namespace pgk

using namespace pgk;

extern "C" {

pgk_status pgk_engine_create(const pgk_model_config_t* cfg, const void* embed, const void* lm_head,
                             const void* final_norm, const pgk_layer_weights_t* layers, pgk_engine* out) {
    PGK_REQUIRE(cfg && embed && final_norm && layers && out, "pgk_engine_create: null argument");
    const auto& c = *cfg;
    PGK_REQUIRE(c.head_dim == 128 || c.head_dim == 64, "pgk_engine_create: head_dim %d not in {64,128}", c.head_dim);
    PGK_REQUIRE(c.num_heads % c.num_kv_heads == 0, "pgk_engine_create: Hq %d %% Hkv %d", c.num_heads, c.num_kv_heads);
    const int G = c.num_heads / c.num_kv_heads;
    PGK_REQUIRE(G >= 1, "pgk_engine_create: GQA group %d", G);
    PGK_REQUIRE(c.hidden_size % 16 == 0 && c.intermediate_size % 16 == 0, "pgk_engine_create: sizes must be multiples of 16");
    PGK_REQUIRE(c.weight_format == 0 || (c.hidden_size % 128 == 0 && c.intermediate_size % 128 == 0),
                "pgk_engine_create: %s weights need hidden_size and intermediate_size multiples of 128 (got %d, %d)",
                c.weight_format == 3 ? "NVF4" : "fp8", c.hidden_size, c.intermediate_size);
    PGK_REQUIRE(c.weight_format >= 0 && c.weight_format <= 3, "pgk_engine_create: weight_format %d not in {0,1,2,3}", c.weight_format);
    if (c.weight_format == 3) {
        // NVF4: every linear needs its codes and scale bytes, 16-byte aligned rows (K/2 bytes each, K % 32 == 0 by the checks above)
        for (int l = 0; l < c.num_layers; ++l) {
            const pgk_layer_weights_t& L = layers[l];
            const void* ptrs[8] = {L.w_qkv, L.s_qkv, L.w_o, L.s_o, L.w_gate_up, L.s_gate_up, L.w_down, L.s_down};
            for (int i = 0; i < 8; ++i)
                PGK_REQUIRE(ptrs[i], "pgk_engine_create: NVF4 layer %d is missing its %s %s", l, i % 2 ? "scales" : "codes",
                            i < 2 ? "qkv" : i < 4 ? "o" : i < 6 ? "gate_up" : "down");
            for (int i = 0; i < 8; i += 2)
                PGK_REQUIRE(((uintptr_t)ptrs[i] & 15) == 0, "pgk_engine_create: NVF4 layer %d codes must be 16-byte aligned", l);
        }
    }
    PGK_REQUIRE(c.max_batch >= 1 && c.max_seq_len >= 1 && c.num_layers >= 1, "pgk_engine_create: bad sizes");
    Engine* e = new Engine();
    e->cfg = c;
    e->embed = (const bf16*)embed;
    e->lm_head = (const bf16*)(lm_head ? lm_head : embed);
    e->final_norm = (const bf16*)final_norm;
    e->layers.assign(layers, layers + c.num_layers);
    int nsplit = (c.max_seq_len + 63) / 64;   // ~64 cached positions per workgroup: one KV batch per wave
    e->cu_count = device_cu_count();
    e->nsplit = nsplit < 1 ? 1 : (nsplit > 64 ? 64 : nsplit);
    e->lm_blocks = 1024;
    // fused attention + o_proj: short contexts, bf16 W_o, and a row slicing that tiles the workgroup
    {
        const int gd = G * c.head_dim, rpp = 256 / (gd / 8);
        int rows = c.hidden_size / 32;
        while (rows > 4 * rpp && rows % 2 == 0) rows /= 2;   // <= 4 preloaded passes per workgroup
        while (rows < rpp) rows *= 2;
        const bool tiles = rows % rpp == 0 && c.hidden_size % rows == 0 && gd / 8 <= 64;
        // PGK_FUSED_ATTN=0: no short-context launch sequence at all (the split-KV sequence at every context; A/B and tests)
        e->short_path = env_on("PGK_FUSED_ATTN");
        e->fused_attn = tiles && c.weight_format == 0 && (G == 1 || G == 2 || G == 4);
        e->oproj_rows = rows;
        e->attn_mfma = c.head_dim == 128 && env_on("PGK_ATTN_MFMA");
        // merged o_proj (long contexts, fp8 W_o): same slicing rule with 16 codes per lane for fp8
        const int nwt = c.weight_format != 0 ? 16 : 8, lpw = gd / nwt, rpp2 = lpw > 0 ? 256 / lpw : 256;
        int rows2 = c.hidden_size / 32;
        while (rows2 > 4 * rpp2 && rows2 % 2 == 0) rows2 /= 2;
        while (rows2 < rpp2) rows2 *= 2;
        e->merged_oproj = env_on("PGK_MERGED_OPROJ") && (G == 1 || G == 2 || G == 4) && lpw >= 8 && lpw <= 64 && 256 % lpw == 0 &&
                          rows2 % rpp2 == 0 && c.hidden_size % rows2 == 0 && (c.weight_format == 0 || (gd % 128 == 0 || 128 % gd == 0)) &&
                          c.weight_format != 3;   // NVF4: the merge kernel + the o_proj GEMV
        e->moproj_rows = rows2;
    }
    const int B = c.max_batch, H = c.hidden_size, D = c.head_dim;
    pgk_status r = PGK_OK;
    auto A = [&](void** p, size_t bytes, size_t* acct) { if (r == PGK_OK) r = dev_alloc(e, p, bytes, acct); };
    const size_t kvb = (size_t)c.num_layers * e->kv_layer_elems() * sizeof(bf16);
    A((void**)&e->kcache, kvb, &e->kv_bytes);
    A((void**)&e->vcache, kvb, &e->kv_bytes);
    A((void**)&e->rope_cos, (size_t)c.max_seq_len * (D / 2) * 4, &e->ws_bytes);
    A((void**)&e->rope_sin, (size_t)c.max_seq_len * (D / 2) * 4, &e->ws_bytes);
    A((void**)&e->cur_cos, (size_t)B * (D / 2) * 4, &e->ws_bytes);
    A((void**)&e->cur_sin, (size_t)B * (D / 2) * 4, &e->ws_bytes);
    A((void**)&e->tokens, (size_t)B * 4, &e->ws_bytes);
    A((void**)&e->positions, (size_t)B * 4, &e->ws_bytes);
    A((void**)&e->token_log, (size_t)e->log_cap * B * 4, &e->ws_bytes);
    A((void**)&e->step_counter, 16, &e->ws_bytes);
    A((void**)&e->h, (size_t)B * H * 4, &e->ws_bytes);
    A((void**)&e->h2, (size_t)B * H * 4, &e->ws_bytes);
    A((void**)&e->qkv, (size_t)B * e->qkv_dim() * 4, &e->ws_bytes);
    A((void**)&e->part, (size_t)B * c.num_heads * e->nsplit * (D + 2) * 4, &e->ws_bytes);
    A((void**)&e->opart, (size_t)B * c.num_kv_heads * H * 4, &e->ws_bytes);
    A((void**)&e->act16, (size_t)B * c.intermediate_size * 2, &e->ws_bytes);
    A((void**)&e->attnv16, (size_t)B * c.num_heads * c.head_dim * 2, &e->ws_bytes);
    A((void**)&e->x16, (size_t)B * H * 2, &e->ws_bytes);
    A((void**)&e->ss_part, (size_t)64 * 1024 * 4, &e->ws_bytes);
    A((void**)&e->attnv, (size_t)B * c.num_heads * D * 4, &e->ws_bytes);
    A((void**)&e->act, (size_t)B * c.intermediate_size * 4, &e->ws_bytes);
    A((void**)&e->logits, (size_t)B * c.vocab_size * 4, &e->ws_bytes);
    e->lm_cap = e->lm_blocks > ceil_div(c.vocab_size, 16) ? e->lm_blocks : ceil_div(c.vocab_size, 16);   // per-sequence argmax partial slots
    {
        const char* ev = getenv("PGK_BATCHED_MFMA");
        e->batched_min = (ev && atoi(ev) == 2) ? 3 : 5;   // 2: from 3 up
        // every projection's K must suit the MFMA decode kernels: K = 128 S with S in {8, 16, 24, 32} (activation
        // fragments in registers) or an LDS image of K x 16 bf16 that fits (K <= 4096); Llama-3-8B's down_proj
        // (K = 14336) does neither, so such models decode batches in GEMV chunks of 8 / 4 / 2 / 1
        auto k_ok = [](int K) { return K % 128 == 0 && K <= 4096; };
        e->batched_mfma = !(ev && atoi(ev) == 0) && k_ok(c.hidden_size) && k_ok(c.intermediate_size) && k_ok(c.num_heads * c.head_dim) &&
                          c.weight_format != 3;   // NVF4: no batched-MFMA form (yet) - batches run as GEMV chunks of <= 8
        // 17..64 sequences in one weight pass (batched_mt_kernel) need K = 128 S with S instantiated; otherwise chunks of 16
        auto k_tiled = [](int K) { const int s = K / 128; return K % 128 == 0 && (s == 2 || s == 4 || s == 8 || s == 16 || s == 24 || s == 32); };
        e->batched_max = (k_tiled(c.hidden_size) && k_tiled(c.intermediate_size) && k_tiled(c.num_heads * c.head_dim)) ? 64 : 16;
        if (const char* em = getenv("PGK_BATCHED_MAX")) { const int v = atoi(em); if (v >= 16 && v < e->batched_max) e->batched_max = v; }
    }
    A((void**)&e->amax_val, (size_t)B * e->lm_cap * 4, &e->ws_bytes);
    A((void**)&e->amax_idx, (size_t)B * e->lm_cap * 4, &e->ws_bytes);
    A((void**)&e->clk_log, (size_t)e->log_cap * 16, &e->ws_bytes);
    if (c.weight_format == 3) {
        const size_t QDn = (size_t)c.num_heads * D, I = c.intermediate_size;
        A((void**)&e->nv_deq, ((size_t)e->qkv_dim() * H + (size_t)H * QDn + 2 * I * H + (size_t)H * I) * 2, &e->ws_bytes);
    }
    {
        // Second, fragment-major copy of the bf16 layer weights: what the short-prompt prefill streams (ops_pkgemm.hip).
        // Costs the layers' bytes again; skipped when that is more than a quarter of the device's free memory.
        const int QDp = c.num_heads * D, NQ = e->qkv_dim(), I = c.intermediate_size;
        const size_t per_layer = ((size_t)NQ * H + (size_t)H * QDp + (size_t)2 * I * H + (size_t)H * I) * 2;
        size_t free_b = 0, total_b = 0;
        const bool fits = hipMemGetInfo(&free_b, &total_b) == hipSuccess && per_layer * c.num_layers < free_b / 4;
        const bool shapes = pkgemm_shape_ok(NQ, H, false) && pkgemm_shape_ok(H, QDp, true) && pkgemm_shape_ok(2 * I, H, false) && pkgemm_shape_ok(H, I, true) && I % 64 == 0;
        // bf16 layers, or fp8 codes + block scales (w8a16): the copy is bf16 either way (ops_pkgemm.hip)
        const bool f8w = c.weight_format == 1;
        // w8a16 engines keep the copy also where the skinny kernels cannot use it (Llama-3-8B: K = 4096 / 14336 is beyond them):
        // their long-prompt GEMMs read it (packed_have), instead of dequantising every weight again in front of every call
        const bool long_only = f8w && !shapes && NQ % 16 == 0 && H % 64 == 0 && QDp % 64 == 0 && I % 64 == 0;
        if (r == PGK_OK && (c.weight_format == 0 || f8w) && (shapes || long_only) && fits && env_on("PGK_PACKED_PREFILL")) {
            e->packed.resize(c.num_layers);
            hipStream_t st = resolve_stream(nullptr);
            for (int l = 0; l < c.num_layers && r == PGK_OK; ++l) {
                auto& P = e->packed[l];
                const auto& L = e->layers[l];
                A((void**)&P.qkv, (size_t)NQ * H * 2, &e->packed_bytes);
                A((void**)&P.o, (size_t)H * QDp * 2, &e->packed_bytes);
                A((void**)&P.gate_up, (size_t)2 * I * H * 2, &e->packed_bytes);
                A((void**)&P.down, (size_t)H * I * 2, &e->packed_bytes);
                if (r == PGK_OK) r = f8w ? pack_weights_fp8(L.w_qkv, L.s_qkv, P.qkv, NQ, H, st) : pack_weights_bf16(L.w_qkv, P.qkv, NQ, H, st);
                if (r == PGK_OK) r = f8w ? pack_weights_fp8(L.w_o, L.s_o, P.o, H, QDp, st) : pack_weights_bf16(L.w_o, P.o, H, QDp, st);
                if (r == PGK_OK) r = f8w ? pack_weights_fp8(L.w_gate_up, L.s_gate_up, P.gate_up, 2 * I, H, st) : pack_weights_bf16(L.w_gate_up, P.gate_up, 2 * I, H, st);
                if (r == PGK_OK) r = f8w ? pack_weights_fp8(L.w_down, L.s_down, P.down, H, I, st) : pack_weights_bf16(L.w_down, P.down, H, I, st);
            }
            if (r == PGK_OK && hipStreamSynchronize(st) != hipSuccess) r = set_error(PGK_ERR_HIP, "pgk_engine_create: packing the prefill weights failed");
            e->packed_have = r == PGK_OK;
            e->packed_ok = e->packed_have && shapes;
            if (e->packed_ok && pkgemm_resid_ok(H, QDp) && pkgemm_resid_ok(H, I)) {
                A((void**)&e->pk_ss, (size_t)128 * PK_SS_LD * 4, &e->ws_bytes);
                e->packed_resid = r == PGK_OK;
            }
            if (e->packed_ok && c.max_batch >= 3 && c.vocab_size % 16 == 0 && H % 32 == 0) {
                A((void**)&e->packed_lm, (size_t)c.vocab_size * H * 2, &e->packed_bytes);
                if (r == PGK_OK) r = pack_weights_bf16(e->lm_head, e->packed_lm, c.vocab_size, H, st);
                if (r == PGK_OK && hipStreamSynchronize(st) != hipSuccess) r = set_error(PGK_ERR_HIP, "pgk_engine_create: packing the lm_head failed");
            }
            if (e->packed_ok && c.max_batch > 16 && env_on("PGK_PACKED_DECODE")) {
                A((void**)&e->dec_slabs, (size_t)16 * 64 * H * 4, &e->ws_bytes);
                e->packed_decode = r == PGK_OK;
            }
        }
    }
    if (r != PGK_OK) { pgk_engine_destroy(e); return r; }
    // RoPE tables in fp32, same formula as the reference (src/pygpukit/llm/layers/rope.py:13-24):
    // freqs = 1/theta^(2i/D) in fp32, angle = float(t) * freq in fp32, cos/sin of that.
    {
        std::vector<float> hc((size_t)c.max_seq_len * (D / 2)), hs(hc.size());
        for (int i = 0; i < D / 2; ++i) {
            const float expo = (float)(2 * i) / (float)D;
            const float freq = 1.0f / powf(c.rope_theta, expo);
            for (int t = 0; t < c.max_seq_len; ++t) {
                const float ang = (float)t * freq;
                hc[(size_t)t * (D / 2) + i] = (float)cos((double)ang);
                hs[(size_t)t * (D / 2) + i] = (float)sin((double)ang);
            }
        }
        hipStream_t st = resolve_stream(nullptr);
        hipError_t he = hipMemcpyAsync(e->rope_cos, hc.data(), hc.size() * 4, hipMemcpyHostToDevice, st);
        if (he == hipSuccess) he = hipMemcpyAsync(e->rope_sin, hs.data(), hs.size() * 4, hipMemcpyHostToDevice, st);
        if (he == hipSuccess) he = hipMemsetAsync(e->kcache, 0, kvb, st);
        if (he == hipSuccess) he = hipMemsetAsync(e->vcache, 0, kvb, st);
        if (he == hipSuccess) he = hipMemsetAsync(e->tokens, 0, (size_t)B * 4, st);
        if (he == hipSuccess) he = hipMemsetAsync(e->positions, 0, (size_t)B * 4, st);
        if (he == hipSuccess) he = hipMemsetAsync(e->step_counter, 0, 16, st);
        if (he == hipSuccess) he = hipMemsetAsync(e->h, 0, (size_t)B * H * 4, st);
        if (he == hipSuccess) he = hipStreamSynchronize(st);
        if (he != hipSuccess) { pgk_engine_destroy(e); return set_error(PGK_ERR_HIP, "pgk_engine_create: %s", hipGetErrorString(he)); }
    }
    *out = e;
    return PGK_OK;
}

pgk_status pgk_engine_destroy(pgk_engine eh) {
    if (!eh) return PGK_OK;
    Engine* e = (Engine*)eh;
    drop_graphs(e);
    for (void* p : e->allocs) (void)pgk_free(p);
    if (e->pf) (void)pgk_free(e->pf);
    if (e->pf_tokens) (void)pgk_free(e->pf_tokens);
    if (e->u_ring) (void)pgk_free(e->u_ring);
    if (e->sampled) (void)pgk_free(e->sampled);
    if (e->sample_scratch) (void)pgk_free(e->sample_scratch);
    delete e;
    return PGK_OK;
}

pgk_status pgk_engine_bytes(pgk_engine eh, size_t* kv_bytes, size_t* workspace_bytes) {
    PGK_REQUIRE(eh, "pgk_engine_bytes: null engine");
    Engine* e = (Engine*)eh;
    if (kv_bytes) *kv_bytes = e->kv_bytes;
    if (workspace_bytes) *workspace_bytes = e->ws_bytes + e->pf_bytes + e->packed_bytes;
    return PGK_OK;
}

pgk_status pgk_engine_set_state(pgk_engine eh, const int32_t* h_tokens, const int32_t* h_positions, int batch, pgk_stream s) {
    PGK_REQUIRE(eh && h_tokens && h_positions, "pgk_engine_set_state: null argument");
    Engine* e = (Engine*)eh;
    PGK_REQUIRE(batch >= 1 && batch <= e->cfg.max_batch, "pgk_engine_set_state: batch %d outside [1,%d]", batch, e->cfg.max_batch);
    for (int b = 0; b < batch; ++b) {
        PGK_REQUIRE(h_tokens[b] >= 0 && h_tokens[b] < e->cfg.vocab_size, "pgk_engine_set_state: token %d out of range", h_tokens[b]);
        PGK_REQUIRE(h_positions[b] >= 0 && h_positions[b] < e->cfg.max_seq_len, "pgk_engine_set_state: position %d outside cache of %d",
                    h_positions[b], e->cfg.max_seq_len);
    }
    hipStream_t st = resolve_stream(s);
    e->pos_hi = 0;
    for (int b = 0; b < batch; ++b) e->pos_hi = h_positions[b] > e->pos_hi ? h_positions[b] : e->pos_hi;
    PGK_CHECK_HIP(hipMemcpyAsync(e->tokens, h_tokens, (size_t)batch * 4, hipMemcpyHostToDevice, st));
    PGK_CHECK_HIP(hipMemcpyAsync(e->positions, h_positions, (size_t)batch * 4, hipMemcpyHostToDevice, st));
    // the residual stream enters a step already holding the embeddings of the state tokens
    embed_kernel<<<batch, 256, 0, st>>>(e->embed, e->tokens, e->h, e->cfg.hidden_size, e->positions, e->rope_cos, e->rope_sin,
                                        e->cur_cos, e->cur_sin, e->cfg.head_dim / 2, e->cfg.max_seq_len);
    PGK_LAUNCH_CHECK();
    PGK_CHECK_HIP(hipStreamSynchronize(st));
    return PGK_OK;
}

pgk_status pgk_engine_decode_step(pgk_engine eh, int batch, pgk_stream s) {
    PGK_REQUIRE(eh, "pgk_engine_decode_step: null engine");
    Engine* e = (Engine*)eh;
    PGK_REQUIRE(batch >= 1 && batch <= e->cfg.max_batch, "pgk_engine_decode_step: batch %d outside [1,%d]", batch, e->cfg.max_batch);
    return enqueue_step(e, batch, resolve_stream(s), 1, &e->launches_per_step);
}

pgk_status pgk_engine_profile_step(pgk_engine eh, int batch, int n_iters, float* h_ms_sum, int* h_count, pgk_stream s) {
    PGK_REQUIRE(eh && h_ms_sum && h_count, "pgk_engine_profile_step: null argument");
    Engine* e = (Engine*)eh;
    PGK_REQUIRE(batch >= 1 && batch <= e->cfg.max_batch && n_iters >= 1, "pgk_engine_profile_step: bad arguments");
    hipStream_t st = resolve_stream(s);
    for (int i = 0; i < KC_COUNT; ++i) { h_ms_sum[i] = 0.f; h_count[i] = 0; }
    // Eager steps whose every launch carries its own start / stop event (hipExtLaunchKernelGGL): the elapsed time of a
    // pair is the dispatch's begin -> end interval, the quantity rocprofv3 --kernel-trace reports - no launch gap, nothing
    // subtracted.
    Probe probe;
    probe.timing = true;
    pgk_status r = PGK_OK;
    for (int it = 0; it < n_iters && r == PGK_OK; ++it) {
        probe.used = 0;
        probe.info.clear();
        r = enqueue_step(e, batch, st, 1, nullptr, &probe);
        if (r != PGK_OK) break;
        hipError_t he = hipStreamSynchronize(st);
        if (he != hipSuccess) { r = set_error(PGK_ERR_HIP, "pgk_engine_profile_step: %s", hipGetErrorString(he)); break; }
        for (size_t i = 0; i < probe.used; ++i) {
            float ms = 0.f;
            const int cls = probe.cls[i];
            if (cls >= 0 && cls < KC_COUNT && hipEventElapsedTime(&ms, probe.ev[2 * i], probe.ev[2 * i + 1]) == hipSuccess) {
                h_ms_sum[cls] += ms;
                h_count[cls] += 1;
            }
        }
    }
    for (hipEvent_t ev : probe.ev) (void)hipEventDestroy(ev);
    return r;
}

// Timeline of ONE replayed step (diagnostic): the step is captured into a temporary graph with every kernel's `tl` slot
// set, replayed `warm` times and then once more; per launch the host gets
//   h_out[6 i .. 6 i + 5] = { kernel class (KC_*), workgroups, first start, last start, first end, last end }
// with the four times in ticks of the 100 MHz s_memrealtime counter relative to the step's first start.  The engine's
// own captured graph is left alone; the sequence state advances by warm + 1 real steps.
pgk_status pgk_engine_timeline(pgk_engine eh, int batch, int warm, uint64_t* h_out, int max_launches, int* n_launches, pgk_stream s) {
    PGK_REQUIRE(eh && h_out && n_launches && max_launches >= 1 && warm >= 0, "pgk_engine_timeline: bad arguments");
    Engine* e = (Engine*)eh;
    PGK_REQUIRE(batch >= 1 && batch <= e->cfg.max_batch, "pgk_engine_timeline: batch %d outside [1,%d]", batch, e->cfg.max_batch);
    hipStream_t st = resolve_stream(s);
    const int cap = 16 * e->cfg.num_layers + 64;
    Probe probe;
    probe.tl_cap = cap;
    const size_t bytes = (size_t)cap * TL_MAXWG * 2 * sizeof(unsigned long long);
    if (pgk_status r = pgk_malloc((void**)&probe.tl, bytes)) return r;
    pgk_status r = PGK_OK;
    hipGraph_t g = nullptr;
    hipGraphExec_t ex = nullptr;
    hipError_t he = hipMemsetAsync(probe.tl, 0, bytes, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    if (he == hipSuccess) he = hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed);
    if (he == hipSuccess) {
        r = enqueue_step(e, batch, st, 0, nullptr, &probe);   // captured: the replays below are what advances the bound
        he = hipStreamEndCapture(st, &g);
    }
    if (r == PGK_OK && he == hipSuccess) he = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    for (int i = 0; r == PGK_OK && he == hipSuccess && i <= warm; ++i) he = hipGraphLaunch(ex, st);
    if (e->pos_hi >= 0) e->pos_hi += warm + 1;
    if (r == PGK_OK && he == hipSuccess) he = hipStreamSynchronize(st);
    const int n = (int)probe.info.size() < cap ? (int)probe.info.size() : cap;
    if (r == PGK_OK && he == hipSuccess) {
        std::vector<unsigned long long> host((size_t)n * TL_MAXWG * 2);
        he = hipMemcpy(host.data(), probe.tl, host.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
        if (he == hipSuccess) {
            unsigned long long origin = ~0ull;
            std::vector<unsigned long long> agg((size_t)n * 4);
            for (int i = 0; i < n; ++i) {
                const int nwg = probe.info[i].nwg < TL_MAXWG ? probe.info[i].nwg : TL_MAXWG;
                unsigned long long s0 = ~0ull, s1 = 0, e0 = ~0ull, e1 = 0;
                for (int w = 0; w < nwg; ++w) {
                    const unsigned long long a = host[((size_t)i * TL_MAXWG + w) * 2], b = host[((size_t)i * TL_MAXWG + w) * 2 + 1];
                    if (a == 0 && b == 0) continue;   // slot never written
                    s0 = a < s0 ? a : s0; s1 = a > s1 ? a : s1; e0 = b < e0 ? b : e0; e1 = b > e1 ? b : e1;
                }
                agg[4 * i] = s0; agg[4 * i + 1] = s1; agg[4 * i + 2] = e0; agg[4 * i + 3] = e1;
                if (s0 < origin) origin = s0;
            }
#ifdef PGK_PHASE_STAMPS
            {
                double sum[KC_COUNT][8] = {}, cnt[KC_COUNT][8] = {}, dur[KC_COUNT] = {};
                for (int i = 0; i < n; ++i) {
                    const int cls = probe.info[i].cls, nwg = probe.info[i].nwg;
                    if (cls < 0 || cls >= KC_COUNT || nwg > 256) continue;
                    for (int w = 0; w < nwg; ++w) {
                        const unsigned long long t0 = host[((size_t)i * TL_MAXWG + w) * 2], t1 = host[((size_t)i * TL_MAXWG + w) * 2 + 1];
                        dur[cls] += (double)(t1 - t0);
                        for (int k = 0; k < 8; ++k) {
                            const unsigned long long v = host[((size_t)i * TL_MAXWG + 256 + 4 * w) * 2 + k];
                            if (v) { sum[cls][k] += (double)(v - t0); cnt[cls][k] += 1; }
                        }
                    }
                }
                for (int cls = 0; cls < KC_COUNT; ++cls)
                    for (int k = 0; k < 8; ++k)
                        if (cnt[cls][k] > 0) fprintf(stderr, "phase stamps: class %d phase %d at %.2f us after its workgroup's start (n=%.0f)\n", cls, k, sum[cls][k] / cnt[cls][k] / 100.0, cnt[cls][k]);
            }
#endif
            *n_launches = n < max_launches ? n : max_launches;
            for (int i = 0; i < *n_launches; ++i) {
                h_out[6 * i] = (uint64_t)probe.info[i].cls;
                h_out[6 * i + 1] = (uint64_t)probe.info[i].nwg;
                for (int k = 0; k < 4; ++k) h_out[6 * i + 2 + k] = agg[4 * i] == ~0ull ? 0 : agg[4 * i + k] - origin;
            }
        }
    }
    if (ex) (void)hipGraphExecDestroy(ex);
    if (g) (void)hipGraphDestroy(g);
    (void)pgk_free(probe.tl);
    if (r != PGK_OK) return r;
    if (he != hipSuccess) return set_error(PGK_ERR_HIP, "pgk_engine_timeline: %s", hipGetErrorString(he));
    return PGK_OK;
}

pgk_status pgk_engine_capture(pgk_engine eh, int batch, pgk_stream s) {
    PGK_REQUIRE(eh, "pgk_engine_capture: null engine");
    Engine* e = (Engine*)eh;
    PGK_REQUIRE(batch >= 1 && batch <= e->cfg.max_batch, "pgk_engine_capture: batch %d outside [1,%d]", batch, e->cfg.max_batch);
    hipStream_t st = resolve_stream(s);
    drop_graphs(e);
    // tier 0: the short-context sequence; then the split-KV sequence once per context tier (1024, 2048, ... positions and the
    // cache length) - needed whenever a context can exceed the short limit (or the short sequences are switched off)
    std::vector<int> spans;
    if (e->short_path) spans.push_back(0);
    if (!e->short_path || e->cfg.max_seq_len > short_limit(batch)) {
        for (int sp = 1024; sp < e->cfg.max_seq_len; sp *= 2) spans.push_back(sp);
        spans.push_back(e->cfg.max_seq_len);
    }
    for (int span : spans) {
        PGK_CHECK_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
        int launches = 0;
        e->step_span = span;
        pgk_status r = decode_step(e, batch, st, &launches, span == 0);
        hipGraph_t g = nullptr;
        hipError_t he = hipStreamEndCapture(st, &g);
        if (r != PGK_OK) { if (g) (void)hipGraphDestroy(g); drop_graphs(e); return r; }
        if (he != hipSuccess || !g) { drop_graphs(e); return set_error(PGK_ERR_HIP, "pgk_engine_capture: hipStreamEndCapture: %s", hipGetErrorString(he)); }
        Engine::Tier t;
        t.span = span; t.graph = g; t.launches = launches;
        he = hipGraphInstantiate(&t.exec, g, nullptr, nullptr, 0);
        e->tiers.push_back(t);      // owned from here on (drop_graphs)
        if (he != hipSuccess) { drop_graphs(e); return set_error(PGK_ERR_HIP, "pgk_engine_capture: hipGraphInstantiate: %s", hipGetErrorString(he)); }
    }
    e->graph_batch = batch;
    e->launches_per_step = e->tiers[pick_tier(e)].launches;
    return PGK_OK;
}

pgk_status pgk_engine_replay(pgk_engine eh, int n_steps, pgk_stream s) {
    PGK_REQUIRE(eh, "pgk_engine_replay: null engine");
    Engine* e = (Engine*)eh;
    PGK_REQUIRE(!e->tiers.empty(), "pgk_engine_replay: no captured graph (call pgk_engine_capture first)");
    hipStream_t st = resolve_stream(s);
    for (int i = 0; i < n_steps; ++i) {
        const auto& t = e->tiers[pick_tier(e)];
        PGK_CHECK_HIP(hipGraphLaunch(t.exec, st));
        e->launches_per_step = t.launches;
        if (e->pos_hi >= 0) ++e->pos_hi;
    }
    return PGK_OK;
}

pgk_status pgk_engine_logits_ptr(pgk_engine eh, void** logits_f32) {
    PGK_REQUIRE(eh && logits_f32, "pgk_engine_logits_ptr: null argument");
    *logits_f32 = ((Engine*)eh)->logits;
    return PGK_OK;
}

pgk_status pgk_engine_read_tokens(pgk_engine eh, int32_t* h_out, int batch, int n_steps, pgk_stream s) {
    PGK_REQUIRE(eh && h_out, "pgk_engine_read_tokens: null argument");
    Engine* e = (Engine*)eh;
    PGK_REQUIRE(n_steps >= 0 && n_steps <= e->log_cap, "pgk_engine_read_tokens: %d steps exceed the log capacity %d", n_steps, e->log_cap);
    PGK_REQUIRE(batch >= 1 && batch <= e->cfg.max_batch, "pgk_engine_read_tokens: bad batch %d", batch);
    hipStream_t st = resolve_stream(s);
    // log rows are max_batch wide; return the first `batch` columns, step-major
    std::vector<int32_t> tmp((size_t)n_steps * e->cfg.max_batch);
    if (n_steps) PGK_CHECK_HIP(hipMemcpyAsync(tmp.data(), e->token_log, tmp.size() * 4, hipMemcpyDeviceToHost, st));
    PGK_CHECK_HIP(hipStreamSynchronize(st));
    for (int t = 0; t < n_steps; ++t)
        for (int b = 0; b < batch; ++b) h_out[(size_t)t * batch + b] = tmp[(size_t)t * e->cfg.max_batch + b];
    return PGK_OK;
}

pgk_status pgk_engine_read_clock(pgk_engine eh, uint64_t* h_out, int n_steps, pgk_stream s) {
    PGK_REQUIRE(eh && h_out, "pgk_engine_read_clock: null argument");
    Engine* e = (Engine*)eh;
    PGK_REQUIRE(n_steps >= 0 && n_steps <= e->log_cap, "pgk_engine_read_clock: %d steps exceed the log capacity %d", n_steps, e->log_cap);
    hipStream_t st = resolve_stream(s);
    if (n_steps) {
        PGK_CHECK_HIP(hipMemcpyAsync(h_out, e->clk_log, (size_t)n_steps * 16, hipMemcpyDeviceToHost, st));
        PGK_CHECK_HIP(hipStreamSynchronize(st));
    }
    return PGK_OK;
}

// In-graph stochastic sampling.  temperature <= 0 restores greedy argmax.  `h_uniforms` [n_rows][max_batch] floats in
// [0,1) are copied into the device ring: step s of the log uses row s % n_rows.  The sampling node and its arguments
// (ring pointer and length, scratch pointer, temperature, top-k, top-p) are baked into a captured graph, so ANY change
// of them - switching sampling on or off, another temperature / top-k / top-p, another n_rows, a scratch buffer that had
// to grow - drops the engine's captured graph: pgk_engine_replay then fails with "no captured graph" until
// pgk_engine_capture is called again.  A refill with the same n_rows and the same parameters only overwrites the ring's
// contents and keeps the graph.
pgk_status pgk_engine_set_sampling(pgk_engine eh, float temperature, int top_k, float top_p, const float* h_uniforms, int n_rows,
                                   pgk_stream s) {
    PGK_REQUIRE(eh, "pgk_engine_set_sampling: null engine");
    Engine* e = (Engine*)eh;
    hipStream_t st = resolve_stream(s);
    auto drop_graph = [&]() {
        if (!e->tiers.empty()) (void)hipStreamSynchronize(st);
        drop_graphs(e);
    };
    if (temperature <= 0.f) {
        if (e->sample_temperature > 0.f) drop_graph();          // a captured sampling node must not be replayed as "greedy"
        e->sample_temperature = 0.f;
        return PGK_OK;
    }
    PGK_REQUIRE(top_k >= 0 && top_p > 0.f && top_p <= 1.f, "pgk_engine_set_sampling: need top_k >= 0 and 0 < top_p <= 1");
    PGK_REQUIRE(h_uniforms && n_rows >= 1, "pgk_engine_set_sampling: uniforms missing");
    const int B = e->cfg.max_batch;
    bool changed = e->sample_temperature != temperature || e->sample_top_k != top_k || e->sample_top_p != top_p || n_rows != e->u_cap;
    if (n_rows > e->u_alloc_rows) {
        drop_graph();                                           // its nodes hold the old ring pointer
        PGK_CHECK_HIP(hipStreamSynchronize(st));
        if (e->u_ring) pgk_free(e->u_ring);
        e->u_ring = nullptr;
        e->u_alloc_rows = 0;
        if (pgk_status r = pgk_malloc((void**)&e->u_ring, (size_t)n_rows * B * 4)) return r;
        e->u_alloc_rows = n_rows;
    }
    if (!e->sampled) {
        if (pgk_status r = pgk_malloc((void**)&e->sampled, (size_t)B * 4)) return r;
    }
    if (const size_t need = sample_scratch_bytes(B, e->cfg.vocab_size, top_k, top_p); need > e->sample_scratch_cap) {
        drop_graph();
        PGK_CHECK_HIP(hipStreamSynchronize(st));
        if (e->sample_scratch) pgk_free(e->sample_scratch);
        e->sample_scratch = nullptr;
        e->sample_scratch_cap = 0;
        if (pgk_status r = pgk_malloc(&e->sample_scratch, need)) return r;
        e->sample_scratch_cap = need;
    }
    if (changed) drop_graph();
    PGK_CHECK_HIP(hipMemcpyAsync(e->u_ring, h_uniforms, (size_t)n_rows * B * 4, hipMemcpyHostToDevice, st));
    PGK_CHECK_HIP(hipStreamSynchronize(st));
    e->u_cap = n_rows;                                          // ring length = rows queued: row index is step % n_rows
    e->sample_temperature = temperature;
    e->sample_top_k = top_k;
    e->sample_top_p = top_p;
    return PGK_OK;
}

pgk_status pgk_engine_reset_log(pgk_engine eh, pgk_stream s) {
    PGK_REQUIRE(eh, "pgk_engine_reset_log: null engine");
    PGK_CHECK_HIP(hipMemsetAsync(((Engine*)eh)->step_counter, 0, 16, resolve_stream(s)));
    return PGK_OK;
}

pgk_status pgk_engine_kv_ptr(pgk_engine eh, int layer, void** k, void** v) {
    PGK_REQUIRE(eh && k && v, "pgk_engine_kv_ptr: null argument");
    Engine* e = (Engine*)eh;
    PGK_REQUIRE(layer >= 0 && layer < e->cfg.num_layers, "pgk_engine_kv_ptr: layer %d", layer);
    *k = e->kcache + (size_t)layer * e->kv_layer_elems();
    *v = e->vcache + (size_t)layer * e->kv_layer_elems();
    return PGK_OK;
}

pgk_status pgk_engine_state_ptr(pgk_engine eh, void** tokens, void** positions) {
    PGK_REQUIRE(eh && tokens && positions, "pgk_engine_state_ptr: null argument");
    *tokens = ((Engine*)eh)->tokens;
    *positions = ((Engine*)eh)->positions;
    return PGK_OK;
}

// Read-only: what the attention of ONE decode step of `batch` sequences whose largest position is `max_position` launches,
// one line per chunk of the step, from the functions the launchers themselves call (next_chunk, attn_flags, attn_choice,
// head_chunk) at the tier pgk_engine_set_state(max_position) + pgk_engine_decode_step - or pgk_engine_replay of a
// capture of the same batch - selects.  Touches neither the device nor the engine's state.
//   chunk b0=<first sequence> m=<sequences> form=gemv|batched|tiled|packed attn=<kernel> heads=<g[+g..]> nsplit=<n> span=<rows> out=f32|bf16 tail=<what follows>
pgk_status pgk_engine_attn_plan(pgk_engine eh, int batch, int max_position, char* out, size_t n) {
    PGK_REQUIRE(eh && out && n > 0, "pgk_engine_attn_plan: null argument");
    const Engine* e = (const Engine*)eh;
    PGK_REQUIRE(batch >= 1 && batch <= e->cfg.max_batch, "pgk_engine_attn_plan: batch %d outside [1,%d]", batch, e->cfg.max_batch);
    PGK_REQUIRE(max_position >= 0 && max_position < e->cfg.max_seq_len, "pgk_engine_attn_plan: position %d outside cache of %d", max_position,
                e->cfg.max_seq_len);
    static const char* const forms[] = {"gemv", "batched", "tiled", "packed"};
    static const char* const kernels[] = {"attn_oproj_mfma", "attn_oproj", "attn_mfma_direct", "attn_decode_direct", "attn_decode_split"};
    static const char* const tails[] = {"none", "merge", "merge_oproj_bf16", "merge_oproj_fp8"};
    const bool short_ctx = step_is_short_at(e, batch, max_position);      // enqueue_step / pick_tier
    // enqueue_step's slicing.  (A replayed SHORT step whose chunk has no whole-context kernel - one sequence with fp8 W_o or a GQA
    // group other than 1 / 2 / 4 - was captured with the cache length as its span instead: same kernels, more slices.)
    const int step_span = span_for_at(e, max_position);
    const int G = e->cfg.num_heads / e->cfg.num_kv_heads;
    size_t used = 0;
    out[0] = 0;
    for (int b0 = 0; b0 < batch;) {
        const ChunkChoice ch = next_chunk(e, batch - b0);
        const AttnFlags af = attn_flags(e, ch.form, ch.m, short_ctx);
        const AttnChoice pick = attn_choice(e, ch.m, step_span, af);
        char heads[64];
        size_t hu = 0;
        for (int off = 0; off < G; off += head_chunk(G, off))
            hu += (size_t)snprintf(heads + hu, hu < sizeof heads ? sizeof heads - hu : 0, "%s%d", off ? "+" : "", head_chunk(G, off));
        const int w = snprintf(out + used, n - used, "chunk b0=%d m=%d form=%s attn=%s heads=%s nsplit=%d span=%d out=%s tail=%s\n", b0, ch.m,
                               forms[ch.form], kernels[pick.kernel], heads, pick.nsplit, pick.span, pick.out_bf16 ? "bf16" : "f32", tails[pick.tail]);
        PGK_REQUIRE(w > 0 && (size_t)w < n - used, "pgk_engine_attn_plan: the plan needs more than %zu bytes", n);
        used += (size_t)w;
        b0 += ch.m;
    }
    return PGK_OK;
}

// Read-only, no device: the request plan of wave `wave` of attn_oproj_mfma_kernel for a context of c1 cached rows, from the
// functions the kernel itself calls (attn_tail_plan.h).  pre: W_o preloads (4 fused, 0 batch form); c0: a later chunk's start.
//   out[0..2] waits of the issue phase: new token, chunk 0 K, chunk 0 V   [3] tiles the loop stages at c0   [4] wait for their K
pgk_status pgk_attn_mfma_plan(int c1, int c0, int wave, int pre, int32_t* out) {
    PGK_REQUIRE(out && c1 >= 0 && wave >= 0 && wave < AM_WAVES && c0 > 0 && c0 % AM_CHUNK == 0 && (pre == 0 || pre == 4), "pgk_attn_mfma_plan: bad argument");
    const int n = c0 < c1 ? am_live_tiles(c0, c1, wave) : 0;      // the loop ends at the first chunk start that is no cached row
    out[0] = am_wait_new(pre);
    out[1] = am_wait_k0(pre);
    out[2] = am_wait_v0(pre);
    out[3] = n;
    out[4] = am_wait_k(n);
    return PGK_OK;
}

// Read-only: what the PROJECTIONS of one decode step (prefill_n == 0: `batch` sequences, largest position `max_position`) or of
// one prefill call of prefill_n tokens launch, from the functions the launchers themselves call (next_chunk, attn_flags,
// gemv_rows / gemv_preload / gemv_grid, batched_is_reg / batched_reg_rows / mt_rows_per_group / mt_tiles / batched_reads_copy,
// pkgemm_pick_splits, prefill_choice).  Touches neither the device nor the engine's state.  Decode: per chunk one line
//   chunk b0=<first sequence> m=<sequences> form=gemv|batched|tiled|packed act=f32|bf16 oproj=fused|merged|own carried=<0|1> normrows=<0|1> attn16=direct|normrows|none
// and one line per projection (qkv, o, gate_up, down, lm_head; o is absent where it runs inside the attention / merge kernel)
//   proj name=<p> kernel=fused_gemv m=<M> act=f32|bf16 w=bf16|fp8|nvf4 pro=norm|plain|norm_sum r=<rows per wave> c=<preload depth> grid=<workgroups> n=<N> k=<K>
//   proj name=<p> kernel=batched_reg|batched_lds|batched_mt w=bf16|fp8 rows=<per workgroup> mp=<LDS image rows> tiles=<M tiles> copy=<0|1> grid=<workgroups> n=<N> k=<K>
//   proj name=<p> kernel=pkgemm|pkgemm_resid splits=<K slabs> n=<N> k=<K>
// Prefill: one line
//   prefill n=<tokens> path=ws|pk|gemm|fp8act ws=.. pk=.. pk_heads=.. carried=.. pkd=.. nvf4=.. fp8act=.. fuse_heads=.. fuse_heads8=.. fuse_sw16=.. fuse_sw8=..
//           s_qkv=.. s_o=.. s_gu=.. s_d=..   (the split-K slabs of the family that runs: wsgemm_nt, pkgemm_nt or engine_gemm_nt_slabs)
pgk_status pgk_engine_linear_plan(pgk_engine eh, int batch, int max_position, int prefill_n, char* out, size_t n) {
    PGK_REQUIRE(eh && out && n > 0, "pgk_engine_linear_plan: null argument");
    const Engine* e = (const Engine*)eh;
    const auto& c = e->cfg;
    size_t used = 0;
    out[0] = 0;
    auto emit = [&](const char* fmt, auto... args) -> bool {
        const int w = snprintf(out + used, n - used, fmt, args...);
        if (w <= 0 || (size_t)w >= n - used) return false;
        used += (size_t)w;
        return true;
    };
    const int H = c.hidden_size, I = c.intermediate_size, QD = c.num_heads * c.head_dim, NQKV = e->qkv_dim(), V = c.vocab_size;
    if (prefill_n > 0) {
        PGK_REQUIRE(prefill_n <= c.max_seq_len, "pgk_engine_linear_plan: %d tokens outside cache of %d", prefill_n, c.max_seq_len);
        const PrefillChoice p = prefill_choice(e, prefill_n);   // engine_prefill.hip
        const char* path = p.fp8act ? "fp8act" : (p.pk ? "pk" : (p.ws ? "ws" : "gemm"));
        const int s_qkv = p.ws && !p.pk ? p.s_qkv : 1, s_gu = p.ws && !p.pk ? p.s_gu : 1;
        const int s_o = p.fp8act ? 1 : (p.pk ? (p.carried ? 1 : p.pk_so) : (p.ws ? p.s_o : p.g_so));
        const int s_d = p.fp8act ? 1 : (p.pk ? (p.carried ? 1 : p.pk_sd) : (p.ws ? p.s_d : p.g_sd));
        PGK_REQUIRE(emit("prefill n=%d path=%s ws=%d pk=%d pk_heads=%d carried=%d pkd=%d nvf4=%d fp8act=%d fuse_heads=%d fuse_heads8=%d fuse_sw16=%d fuse_sw8=%d "
                         "s_qkv=%d s_o=%d s_gu=%d s_d=%d\n", prefill_n, path, (int)p.ws, (int)p.pk, (int)p.pk_heads, (int)p.carried, (int)p.pkd, (int)p.nv4,
                         (int)p.fp8act, (int)p.fuse_heads, (int)p.fuse_heads8, (int)p.fuse_sw16, (int)p.fuse_sw8, s_qkv, s_o, s_gu, s_d),
                    "pgk_engine_linear_plan: the plan needs more than %zu bytes", n);
        return PGK_OK;
    }
    PGK_REQUIRE(batch >= 1 && batch <= c.max_batch, "pgk_engine_linear_plan: batch %d outside [1,%d]", batch, c.max_batch);
    PGK_REQUIRE(max_position >= 0 && max_position < c.max_seq_len, "pgk_engine_linear_plan: position %d outside cache of %d", max_position, c.max_seq_len);
    static const char* const forms[] = {"gemv", "batched", "tiled", "packed"};
    const bool short_ctx = step_is_short_at(e, batch, max_position) && e->short_path;      // enqueue_step / decode_step
    const bool fp8 = c.weight_format == 1 || c.weight_format == 2;
    const int nw = c.weight_format == 3 ? GEMV_NW_NVF4 : (fp8 ? GEMV_NW_FP8 : GEMV_NW_BF16);   // decode_step: WT
    const char* wname = c.weight_format == 3 ? "nvf4" : (fp8 ? "fp8" : "bf16");
    bool ok = true;
    for (int b0 = 0; b0 < batch && ok;) {
        const ChunkChoice ch = next_chunk(e, batch - b0);
        const AttnFlags af = attn_flags(e, ch.form, ch.m, short_ctx);
        const int M = ch.m;
        if (ch.form == CF_GEMV) {
            const bool partials = af.fused || af.merged;                  // decode_chunk
            const char* act = M >= 4 ? "bf16" : "f32";                    // decode_step_impl: XT
            ok = emit("chunk b0=%d m=%d form=gemv act=%s oproj=%s carried=0 normrows=0 attn16=none\n", b0, M, act, af.fused ? "fused" : (af.merged ? "merged" : "own"));
            auto gemv = [&](const char* name, int wnw, const char* wn, const char* pro, bool swiglu, int n_out, int K, int r, int force_grid) {
                if (r == 0) r = gemv_rows(wnw, M, swiglu, n_out, K);      // launch_fused_auto
                ok = ok && emit("proj name=%s kernel=fused_gemv m=%d act=%s w=%s pro=%s r=%d c=%d grid=%d n=%d k=%d\n", name, M, act, wn, pro, r,
                                gemv_preload(wnw, r, K), gemv_grid(r, swiglu, n_out, force_grid), n_out, K);
            };
            gemv("qkv", nw, wname, "norm", false, NQKV, H, 0, 0);
            if (!partials) gemv("o", nw, wname, "plain", false, H, QD, 0, 0);
            gemv("gate_up", nw, wname, partials && M <= 2 ? "norm_sum" : "norm", true, I, H, 0, 0);
            gemv("down", nw, wname, "plain", false, H, I, 0, 0);
            gemv("lm_head", GEMV_NW_BF16, "bf16", "norm", false, V, H, 4, e->lm_blocks);
        } else if (ch.form == CF_PACKED) {
            const bool carried = e->packed_resid;                          // decode_chunk_packed
            ok = emit("chunk b0=%d m=%d form=packed act=bf16 oproj=own carried=%d normrows=0 attn16=%s\n", b0, M, carried ? 1 : 0, af.direct ? "direct" : "normrows");
            ok = ok && emit("proj name=qkv kernel=pkgemm splits=1 n=%d k=%d\n", NQKV, H);
            ok = ok && emit("proj name=o kernel=%s splits=%d n=%d k=%d\n", carried ? "pkgemm_resid" : "pkgemm", carried ? 1 : pkgemm_pick_splits(M, H, QD), H, QD);
            ok = ok && emit("proj name=gate_up kernel=pkgemm splits=1 n=%d k=%d\n", 2 * I, H);
            ok = ok && emit("proj name=down kernel=%s splits=%d n=%d k=%d\n", carried ? "pkgemm_resid" : "pkgemm", carried ? 1 : pkgemm_pick_splits(M, H, I), H, I);
            const int rows = mt_rows_per_group(V, true);
            ok = ok && emit("proj name=lm_head kernel=batched_mt w=bf16 rows=%d mp=0 tiles=%d copy=%d grid=%d n=%d k=%d\n", rows, mt_tiles(M),
                            batched_reads_copy(false, rows, e->packed_lm != nullptr) ? 1 : 0, batched_lm_blocks(V), V, H);
        } else {
            const bool tiled = ch.form == CF_TILED;                        // decode_chunk_batched
            ok = emit("chunk b0=%d m=%d form=%s act=bf16 oproj=own carried=0 normrows=%d attn16=%s\n", b0, M, forms[ch.form], tiled ? 1 : 0,
                      af.direct ? "direct" : (tiled ? "normrows" : "none"));
            auto bat = [&](const char* name, bool wfp8, bool logits, bool have_copy, int N, int K) {
                const char* wn = wfp8 ? "fp8" : "bf16";
                if (tiled) {             // launch_batched_tiled
                    const int rows = mt_rows_per_group(N, logits);
                    ok = ok && emit("proj name=%s kernel=batched_mt w=%s rows=%d mp=0 tiles=%d copy=%d grid=%d n=%d k=%d\n", name, wn, rows, mt_tiles(M),
                                    batched_reads_copy(wfp8, rows, have_copy) ? 1 : 0, logits ? batched_lm_blocks(V) : ceil_div(N, rows), N, K);
                } else if (batched_is_reg(K)) {   // launch_batched: the register-fragment kernel
                    const int rows = batched_reg_rows(N, logits);
                    ok = ok && emit("proj name=%s kernel=batched_reg w=%s rows=%d mp=0 tiles=1 copy=%d grid=%d n=%d k=%d\n", name, wn, rows,
                                    batched_reads_copy(wfp8, rows, have_copy) ? 1 : 0, logits ? batched_lm_blocks(V) : ceil_div(N, rows), N, K);
                } else {
                    ok = ok && emit("proj name=%s kernel=batched_lds w=%s rows=16 mp=%d tiles=1 copy=0 grid=%d n=%d k=%d\n", name, wn, M <= 8 ? 8 : 16,
                                    logits ? batched_lm_blocks(V) : ceil_div(N, 16), N, K);
                }
            };
            const bool lcopy = batched_layer_copy(e, fp8);
            bat("qkv", fp8, false, lcopy, NQKV, H);
            bat("o", fp8, false, false, H, QD);
            bat("gate_up", fp8, false, lcopy, I, H);
            bat("down", fp8, false, false, H, I);
            bat("lm_head", false, true, e->packed_lm != nullptr, V, H);
        }
        b0 += ch.m;
    }
    PGK_REQUIRE(ok, "pgk_engine_linear_plan: the plan needs more than %zu bytes", n);
    return PGK_OK;
}

pgk_status pgk_engine_launches_per_step(pgk_engine eh, int* n) {
    PGK_REQUIRE(eh && n, "pgk_engine_launches_per_step: null argument");
    *n = ((Engine*)eh)->launches_per_step;
    return PGK_OK;
}

}  // extern "C"
