// Prefill of the native engine (bf16 activations, fp32 residual stream), its own translation unit like engine_batched.hip;
// the decode step's packed path shares two host entries with it (rmsnorm_slabs, packed_mlp_carried: engine_state.hip.h).

#include "attn_plan.h"
#include "engine_gemv.hip.h"
#include "engine_state.hip.h"
#include "gemm_epilogues.hip.h"
#include "gemm_plan.h"      // wsgemm_pick_splits
#include "pkgemm.hip.h"

namespace pgk {

pgk_status engine_gemm_nt(const bf16* A, const void* W, const bf16* wscale, bool fp8, void* C, bool accum_f32, int M,
                          int N, int K, hipStream_t st, bool packed = false);      // packed: W = the fragment-major bf16 copy
bool engine_gemm_packed_ok(int M, int N, int K);
int engine_gemm_pick_splits(int M, int N, int K);
pgk_status engine_gemm_nt_slabs(const bf16* A, const void* W, float* slabs, int splits, int M, int N, int K, hipStream_t st, bool packed = false);
pgk_status gemm_fp8_nt(const uint8_t* a, const float* sa, const uint8_t* w, const bf16* sw, void* c, bool accum_f32, int M,
                       int N, int K, hipStream_t st);
pgk_status quantize_fp8_rows_bf16(const bf16* x, uint8_t* out, float* scale, int M, int K, hipStream_t st);
bool engine_gemm_qkv_heads_ok(int M, int N, int K);            // ops_gemm.hip: QKV projection with per-head norm + RoPE + cache write as its epilogue
pgk_status engine_gemm_qkv_heads_nt(const bf16* A, const bf16* W, bf16* qkv, int M, int N, int K, const QkvHeadArgs& hd, hipStream_t st, bool packed = false);
bool engine_gemm_swiglu_ok(int M, int I, int K, bool fp8);     // ops_gemm.hip: gate / up projection with the SwiGLU epilogue
pgk_status engine_gemm_swiglu_nt(const bf16* A, const void* W, const bf16* wscale, bool fp8, bf16* act, int M, int I, int K, hipStream_t st, bool packed = false);
bool gemm_fp8_qkv_heads_ok(int M, int N, int K);               // ops_fp8_gemm.hip: the same epilogue on the fp8 x fp8 256-tile kernel
pgk_status gemm_fp8_qkv_heads_nt(const uint8_t* a, const float* sa, const uint8_t* w, const bf16* sw, bf16* qkv, int M, int N, int K,
                                 const QkvHeadArgs& hd, hipStream_t st);
bool gemm_fp8_swiglu_ok(int M, int I, int K);                  // ops_fp8_gemm.hip: ... and the e4m3 quantisation of the result
pgk_status gemm_fp8_swiglu_nt(const uint8_t* a, const float* sa, const uint8_t* w, const bf16* sw, uint8_t* q_out, float* s_out, int M, int I,
                              int K, hipStream_t st);
pgk_status wsgemm_nt(const bf16* a, int lda, const void* w, const bf16* wscale, bool fp8, void* c, const bf16* bias, int mode,
                     int splits, int M, int N, int K, hipStream_t st);
pgk_status dequant_nvf4_nk(const uint8_t* data, const uint8_t* scale, bf16* out, int n, int k, hipStream_t st);   // ops_nvf4.hip

__global__ void embed_rows_kernel(const bf16* embed, const int32_t* tokens, float* h, int H) {
    const int s = blockIdx.x;
    const bf16* row = embed + (size_t)tokens[s] * H;
    for (int i = threadIdx.x; i < H; i += blockDim.x) h[(size_t)s * H + i] = to_f(row[i]);
}

// Up to EMBED_ARG_TOKENS token ids travel by value in the kernel arguments (512 bytes): no host-to-device copy of the ids,
// no synchronise for the caller's (possibly pageable) buffer and no launch into a stream that just went idle.
constexpr int EMBED_ARG_TOKENS = 128;
struct EmbedTokenArgs { int32_t id[EMBED_ARG_TOKENS]; };
__global__ void embed_rows_arg_kernel(const bf16* embed, float* h, int H, EmbedTokenArgs tokens) {
    const int s = blockIdx.x;
    const bf16* row = embed + (size_t)tokens.id[s] * H;
    for (int i = threadIdx.x; i < H; i += blockDim.x) h[(size_t)s * H + i] = to_f(row[i]);
}

// h32[s] += sum of the split-K slabs of the projection that precedes this norm (if any), written back;
// x_bf16[s] = rmsnorm(h32[s]) * gamma.  One 256-thread workgroup per row, 4 elements per thread per trip;
// the slab loads are unconditional (clamped slab index, masked add) so they share one memory round trip.
// With q8 != nullptr (fp8-activation prefill, H % 128 == 0) the row leaves as e4m3 codes + one fp32 scale per 128
// columns instead of bf16: the values quantised are the bf16-rounded ones, so this is bit-identical to
// rmsnorm -> quantize_rows_kernel without the second pass over the activations.  (The caller asks for it only with
// H <= 4096 - prefill_choice's fuse_q - so the e4m3 branch of the loop over the columns past 4096 has never run.)
template <int NS>   // slab loads issued per trip (>= nslabs): 4 on the packed path, 16 covers every split count of wsgemm
__global__ __launch_bounds__(256) void rmsnorm_f32_bf16_kernel(float* h, const bf16* gamma, bf16* out, int rows, int H,
                                                               float eps, const float* slabs, int nslabs,
                                                               uint8_t* q8 = nullptr, float* q8s = nullptr) {
    __shared__ float red[16];
    const int row = blockIdx.x;
    float* hr = h + (size_t)row * H;
    constexpr int MAXT = 4;                     // columns below 4096 stay in registers between the two passes
    float4 v[MAXT];
    uint2 gm[MAXT];                             // gamma requested with the row: not a second round trip after the reduction
    float ss = 0.f;
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
        const int i = (threadIdx.x + t * 256) * 4;
        gm[t] = *reinterpret_cast<const uint2*>(gamma + min(i, H - 4));
    }
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
        const int i = (threadIdx.x + t * 256) * 4;
        if (i < H) {                            // block-uniform per t when H % 1024 == 0; otherwise per-lane tail
            float4 acc = *reinterpret_cast<const float4*>(hr + i);
            if (nslabs > 0) {
                float4 p[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s)
                    p[s] = *reinterpret_cast<const float4*>(slabs + ((size_t)min(s, nslabs - 1) * rows + row) * H + i);
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const float w = s < nslabs ? 1.f : 0.f;
                    acc.x = fmaf(w, p[s].x, acc.x); acc.y = fmaf(w, p[s].y, acc.y);
                    acc.z = fmaf(w, p[s].z, acc.z); acc.w = fmaf(w, p[s].w, acc.w);
                }
                *reinterpret_cast<float4*>(hr + i) = acc;
            }
            v[t] = acc;
            ss += acc.x * acc.x + acc.y * acc.y + acc.z * acc.z + acc.w * acc.w;
        }
    }
    // columns past 4096 (as norm_rows_bf16_kernel): slabs added and the row written back here, summed, re-read below
    for (int i = (threadIdx.x + MAXT * 256) * 4; i < H; i += 1024) {
        float4 acc = *reinterpret_cast<const float4*>(hr + i);
        if (nslabs > 0) {
            for (int s = 0; s < nslabs; ++s) {
                const float4 p = *reinterpret_cast<const float4*>(slabs + ((size_t)s * rows + row) * H + i);
                acc.x += p.x; acc.y += p.y; acc.z += p.z; acc.w += p.w;
            }
            *reinterpret_cast<float4*>(hr + i) = acc;         // read back below by the thread that wrote it
        }
        ss += acc.x * acc.x + acc.y * acc.y + acc.z * acc.z + acc.w * acc.w;
    }
    ss = block_sum(ss, red);
    const float inv = 1.0f / sqrtf(ss / H + eps);
    auto emit = [&](int i, const float4& u, const uint2& g) {
        const float g0 = __uint_as_float(g.x << 16), g1 = __uint_as_float(g.x & 0xFFFF0000u);
        const float g2 = __uint_as_float(g.y << 16), g3 = __uint_as_float(g.y & 0xFFFF0000u);
        uint2 o;
        o.x = pack_bf16x2(u.x * inv * g0, u.y * inv * g1);
        o.y = pack_bf16x2(u.z * inv * g2, u.w * inv * g3);
        if (q8) {   // 32 lanes x 4 columns = one 128-column scale block
            const float f0 = __uint_as_float(o.x << 16), f1 = __uint_as_float(o.x & 0xFFFF0000u);
            const float f2 = __uint_as_float(o.y << 16), f3 = __uint_as_float(o.y & 0xFFFF0000u);
            float amax = fmaxf(fmaxf(fabsf(f0), fabsf(f1)), fmaxf(fabsf(f2), fabsf(f3)));
            amax = group16_max(amax);
            amax = fmaxf(amax, __shfl_xor(amax, 16, 64));
            const float sc = amax > 0.f ? amax / 448.0f : 1.0f;
            *reinterpret_cast<uint32_t*>(q8 + (size_t)row * H + i) = pack_fp8x4(f0 / sc, f1 / sc, f2 / sc, f3 / sc);
            if ((threadIdx.x & 31) == 0) q8s[(size_t)row * (H >> 7) + (i >> 7)] = sc;
        } else {
            *reinterpret_cast<uint2*>(out + (size_t)row * H + i) = o;
        }
    };
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
        const int i = (threadIdx.x + t * 256) * 4;
        if (i < H) emit(i, v[t], gm[t]);
    }
    for (int i = (threadIdx.x + MAXT * 256) * 4; i < H; i += 1024)
        emit(i, *reinterpret_cast<const float4*>(hr + i), *reinterpret_cast<const uint2*>(gamma + i));
}

// Per (token s, head slot hh) of qkv[n][(Hq+2Hkv)*D] bf16: q heads -> norm+rope in place;
// k heads -> norm+rope -> cache row; v heads -> cache row.  One lane-group of D/8 lanes per vector.
template <int D>
__global__ __launch_bounds__(256) void qknorm_rope_kvwrite_kernel(bf16* qkv, const bf16* q_gamma, const bf16* k_gamma,
                                                                  float eps, const float* rope_cos,
                                                                  const float* rope_sin, bf16* kcache, bf16* vcache,
                                                                  int n, int hq, int hkv, int max_seq, int start_pos,
                                                                  const float* slabs, int nslabs) {
    constexpr int LPR = D / 8, HALF = D / 2, VPB = 256 / LPR;
    const int nslots = hq + 2 * hkv;
    const long long vec = (long long)blockIdx.x * VPB + threadIdx.x / LPR;
    const int sub = threadIdx.x % LPR;
    const bool live = vec < (long long)n * nslots;
    const long long vv = live ? vec : 0;
    const int s = (int)(vv / nslots), hh = (int)(vv % nslots);
    bf16* src = qkv + (size_t)s * nslots * D + (size_t)hh * D + sub * 8;
    float x[8];
    Vec<bf16> raw;
    if (nslabs > 0) {
        // the projection arrived as split-K fp32 partials: sum them and round to bf16, as the projection's
        // own bf16 store would have
        const size_t off = (size_t)s * nslots * D + (size_t)hh * D + sub * 8, stride = (size_t)n * nslots * D;
        float4 a0 = *reinterpret_cast<const float4*>(slabs + off), a1 = *reinterpret_cast<const float4*>(slabs + off + 4);
        for (int k = 1; k < nslabs; ++k) {
            const float4 b0 = *reinterpret_cast<const float4*>(slabs + k * stride + off);
            const float4 b1 = *reinterpret_cast<const float4*>(slabs + k * stride + off + 4);
            a0.x += b0.x; a0.y += b0.y; a0.z += b0.z; a0.w += b0.w;
            a1.x += b1.x; a1.y += b1.y; a1.z += b1.z; a1.w += b1.w;
        }
        const float f[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        raw.from_float(f);
    } else {
        raw.load(src);
    }
    raw.to_float(x);
    const int pos = start_pos + s;
    const bool is_q = hh < hq, is_k = !is_q && hh < hq + hkv;
    if (is_q || is_k) {
        const bf16* gamma = is_q ? q_gamma : k_gamma;
        if (gamma) {
            float ss = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) ss = fmaf(x[j], x[j], ss);
            ss = group_sum<LPR>(ss);
            const float inv = 1.0f / sqrtf(ss / D + eps);
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = x[j] * inv * to_f(gamma[sub * 8 + j]);
        }
        const bool lo = sub < LPR / 2;
        const float* cs = rope_cos + (size_t)min(pos, max_seq - 1) * HALF;
        const float* sn = rope_sin + (size_t)min(pos, max_seq - 1) * HALF;
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float other = xor_half<LPR>(x[j]);
            const int dd = (sub * 8 + j) % HALF;
            o[j] = lo ? (x[j] * cs[dd] - other * sn[dd]) : (x[j] * cs[dd] + other * sn[dd]);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = o[j];
    }
    if (!live) return;
    Vec<bf16> ov;
    ov.from_float(x);
    if (is_q) {
        ov.store(src);
    } else if (pos < max_seq) {
        const int kvh = is_k ? hh - hq : hh - hq - hkv;
        bf16* dst = (is_k ? kcache : vcache) + ((size_t)kvh * max_seq + pos) * D + sub * 8;
        ov.store(dst);
    }
}

// act[s][i] = silu(gu[s][i]) * gu[s][I+i]   (bf16 in/out, fp32 math)
// With nslabs > 0 the gate_up projection arrives as split-K fp32 partials [nslabs][n][2I] (summed, rounded to bf16).
// q8 != nullptr (I % 128 == 0): e4m3 codes + per-(row, 128 columns) scales of the bf16-rounded result instead of bf16
__global__ void swiglu_rows_kernel(const bf16* gu, bf16* act, int n, int I, const float* slabs, int nslabs, uint8_t* q8 = nullptr,
                                   float* q8s = nullptr) {
    const size_t total = (size_t)n * I / 8;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += stride) {
        const size_t s = t / (I / 8), c = t % (I / 8);
        Vec<bf16> g, u;
        if (nslabs > 0) {
            const size_t og = s * 2 * I + c * 8, ou = og + I, sst = (size_t)n * 2 * I;
            float sg[8], su[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) { sg[j] = 0.f; su[j] = 0.f; }
            for (int k = 0; k < nslabs; ++k) {
                const float4 g0 = *reinterpret_cast<const float4*>(slabs + k * sst + og), g1 = *reinterpret_cast<const float4*>(slabs + k * sst + og + 4);
                const float4 u0 = *reinterpret_cast<const float4*>(slabs + k * sst + ou), u1 = *reinterpret_cast<const float4*>(slabs + k * sst + ou + 4);
                sg[0] += g0.x; sg[1] += g0.y; sg[2] += g0.z; sg[3] += g0.w; sg[4] += g1.x; sg[5] += g1.y; sg[6] += g1.z; sg[7] += g1.w;
                su[0] += u0.x; su[1] += u0.y; su[2] += u0.z; su[3] += u0.w; su[4] += u1.x; su[5] += u1.y; su[6] += u1.z; su[7] += u1.w;
            }
            g.from_float(sg);
            u.from_float(su);
        } else {
            g.load(gu + s * 2 * I + c * 8);
            u.load(gu + s * 2 * I + I + c * 8);
        }
        g = swiglu8(g, u);
        if (q8) {   // 16 lanes x 8 columns = one scale block; total and stride are multiples of 16, so groups stay whole
            float sc;
            const uint2 o = quant_e4m3_block16(g, sc);
            *reinterpret_cast<uint2*>(q8 + s * I + c * 8) = o;
            if ((c & 15) == 0) q8s[s * (I >> 7) + (c >> 4)] = sc;
        } else {
            g.store(act + s * I + c * 8);
        }
    }
}

__global__ void bf16_rows_to_f32_kernel(const bf16* in, float* out, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += stride) out[i] = to_f(in[i]);
}

pgk_status rmsnorm_slabs(float* h, const bf16* gamma, bf16* x, int rows, int H, float eps, const float* slabs, int* pending, uint8_t* q8,
                         float* q8s, hipStream_t st, int* launches) {
    const auto kfn = *pending <= 4 ? rmsnorm_f32_bf16_kernel<4> : rmsnorm_f32_bf16_kernel<16>;
    kfn<<<rows, 256, 0, st>>>(h, gamma, x, rows, H, eps, slabs, *pending, q8, q8s);
    *pending = 0;
    PGK_LAUNCH_CHECK();
    return counted(launches, PGK_OK);
}

// o_proj adds the residual itself and leaves bf16(h * gamma_mlp) + row statistics; gate_up scales by 1 / rms;
// down_proj does the same for the next layer's attention norm: 5 launches per layer with QKV and attention
pgk_status packed_mlp_carried(Engine* e, int layer, int rows, const bf16* attn16, bf16* act16, float* h, bf16* x16, int* ss_n, hipStream_t st,
                              int* launches) {
    const auto& c = e->cfg;
    const int H = c.hidden_size, I = c.intermediate_size, QD = c.num_heads * c.head_dim;
    const auto& P = e->packed[layer];
    if (pgk_status r = counted(launches, pkgemm_resid_nt(attn16, QD, P.o, h, rows, H, QD, (const bf16*)e->layers[layer].mlp_norm, x16, e->pk_ss, ss_n, st))) return r;
    mark(KC_GATEUP);
    PkArgs gn{};
    gn.ss_in = e->pk_ss; gn.ss_n = *ss_n; gn.ss_eps = c.norm_eps;
    if (pgk_status r = counted(launches, pkgemm_nt(x16, H, P.gate_up, act16, I, PK_EPI_SWIGLU, 1, rows, 2 * I, H, &gn, st))) return r;
    mark(KC_DOWN);
    const bf16* gnext = layer + 1 < c.num_layers ? (const bf16*)e->layers[layer + 1].attn_norm : nullptr;
    return counted(launches, pkgemm_resid_nt(act16, I, P.down, h, rows, H, I, gnext, x16, e->pk_ss, ss_n, st));
}

// pgk_engine_prefill's choices for a chunk of n tokens, as a pure function of the engine's host state (and the
// PGK_FUSED_EPILOGUES switch, read per call as before): pgk_engine_prefill executes them, pgk_engine_linear_plan prints them.
PrefillChoice prefill_choice(const Engine* e, int n) {
    const auto& c = e->cfg;
    const int H = c.hidden_size, I = c.intermediate_size, D = c.head_dim, QD = c.num_heads * D, NQKV = e->qkv_dim();
    PrefillChoice p{};
    // split-K slabs of the N = hidden projections on the weight-streaming path (n <= 128)
    const bool ws = p.ws = n <= 128;
    p.s_o = ws ? wsgemm_pick_splits(H, QD, true) : 1; p.s_d = ws ? wsgemm_pick_splits(H, I, true) : 1;
    p.s_qkv = ws ? wsgemm_pick_splits(NQKV, H, true) : 1; p.s_gu = ws ? wsgemm_pick_splits(2 * I, H, true) : 1;
    // packed-weight path (ops_pkgemm.hip): bf16 layers, n <= 128; its own split counts for the N = hidden projections
    const bool pk = p.pk = ws && e->packed_ok;
    p.pk_so = pk ? pkgemm_pick_splits(n, H, QD) : 1; p.pk_sd = pk ? pkgemm_pick_splits(n, H, I) : 1;
    p.pk_heads = pk && D == 128;       // QKV epilogue: per-head norm + RoPE + cache write inside the projection
    p.carried = pk && e->packed_resid; // o_proj / down_proj carry the next RMSNorm
    // long prompts, bf16 weights: the N = hidden projections as split-K slabs when their 128-tiles do not cover the chip
    // (QKV / gate_up were tried too - their consumers can sum slabs - and measured slightly slower: 3.06 vs 2.99 ms at S = 512)
    // w8a16 engines, long prompts: the staged bf16 GEMMs read the DEQUANTISED fragment-major copy the engine already holds
    // (pack_weights_fp8: bf16(code x scale), the value the reference's w8a16 GEMM multiplies) - same kernels, epilogues and
    // times as a bf16 engine (S = 512: 4.23 -> 2.44 ms) instead of the in-staging-dequant 128-tile kernel / a per-call
    // dequantisation pass in front of the 256-tile kernel
    const bool pkd = p.pkd = !ws && c.weight_format == 1 && e->packed_have && engine_gemm_packed_ok(n, NQKV, H) && engine_gemm_packed_ok(n, H, QD) &&
                             engine_gemm_packed_ok(n, 2 * I, H) && engine_gemm_packed_ok(n, H, I);
    p.nv4 = c.weight_format == 3;                 // NVF4: each layer's linears dequantised to bf16 (e->nv_deq), then the bf16 engine's path
    const bool w16 = p.w16 = c.weight_format == 0 || p.nv4;   // the projections read bf16 row-major weights
    const bool gsplit = p.gsplit = !ws && (w16 || pkd);
    p.g_so = gsplit ? engine_gemm_pick_splits(n, H, QD) : 1; p.g_sd = gsplit ? engine_gemm_pick_splits(n, H, I) : 1;
    const bool fp8 = p.fp8 = c.weight_format == 1 || c.weight_format == 2;
    const bool fp8act = p.fp8act = c.weight_format == 2 && n > 128;   // fp8 x fp8 MFMA projections, activations quantised on the fly
    // (PGK_FUSED_EPILOGUES=0 keeps the separate passes - quantise, SwiGLU: the A/B switch of the bit-identity tests)
    const bool fuse_epi = p.fuse_epi = env_on("PGK_FUSED_EPILOGUES");
    const bool fuse_q = p.fuse_q = fp8act && H % 128 == 0 && I % 128 == 0 && H <= 4096 && fuse_epi;
    // SwiGLU in the gate / up GEMM's epilogue (256-tile kernels; fp8 x fp8: with the quantisation of its result)
    p.fuse_sw8 = fuse_q && gemm_fp8_swiglu_ok(n, I, H);
    p.fuse_sw16 = !fp8act && !ws && fuse_epi && engine_gemm_swiglu_ok(n, I, H, fp8 && !pkd);
    // per-head norm + RoPE + cache write in the QKV GEMM's epilogue (bf16 weights, head_dim 128, 128-tile kernel: tile column = head)
    p.fuse_heads8 = fuse_q && D == 128 && gemm_fp8_qkv_heads_ok(n, NQKV, H);      // fp8 x fp8: x's codes are already in q8
    p.fuse_heads = p.fuse_heads8 || (!ws && !pk && fuse_epi && (w16 || pkd) && D == 128 && engine_gemm_qkv_heads_ok(n, NQKV, H));
    return p;
}

// the per-head norm + RoPE + cache write arguments of a QKV projection's epilogue (PkArgs, QkvHeadArgs)
template <class HeadArgs>
static void fill_head_args(HeadArgs& hd, const Engine* e, const pgk_layer_weights_t& L, bf16* kc, bf16* vc, int start_pos) {
    const auto& c = e->cfg;
    hd.q_gamma = c.use_qk_norm ? (const bf16*)L.q_norm : nullptr;
    hd.k_gamma = c.use_qk_norm ? (const bf16*)L.k_norm : nullptr;
    hd.eps = c.norm_eps; hd.rope_cos = e->rope_cos; hd.rope_sin = e->rope_sin; hd.kcache = kc; hd.vcache = vc;
    hd.hq = c.num_heads; hd.hkv = c.num_kv_heads; hd.max_seq = c.max_seq_len; hd.start_pos = start_pos;
}

}  // namespace pgk

using namespace pgk;

extern "C" {

pgk_status pgk_engine_prefill(pgk_engine eh, int seq, const int32_t* h_tokens, int n, int start_pos, void* all_logits,
                              float* h_last_logits, pgk_stream s) {
    PGK_REQUIRE(eh && h_tokens, "pgk_engine_prefill: null argument");
    Engine* e = (Engine*)eh;
    const auto& c = e->cfg;
    PGK_REQUIRE(seq >= 0 && seq < c.max_batch, "pgk_engine_prefill: sequence slot %d outside [0,%d)", seq, c.max_batch);
    PGK_REQUIRE(n >= 1 && start_pos >= 0 && start_pos + n <= c.max_seq_len, "pgk_engine_prefill: positions %d..%d outside cache of %d",
                start_pos, start_pos + n, c.max_seq_len);
    hipStream_t st = resolve_stream(s);
    // (prompts of 129..256 tokens used to run as two chunks of <= 128 through the packed-weight kernels; since the staged 128-tile
    // GEMM and the epilogue fusions of round 3 the long-prompt path is faster at every such length: 144 tokens 1.94 vs 2.38 ms,
    // 256 tokens 2.27 vs 2.62)
    const int H = c.hidden_size, I = c.intermediate_size, D = c.head_dim, QD = c.num_heads * D, NQKV = e->qkv_dim();
    // which kernels the projections run on, their split-K slabs and epilogues: prefill_choice, above (also what
    // pgk_engine_linear_plan prints)
    const PrefillChoice pc = prefill_choice(e, n);
    const bool ws = pc.ws, pk = pc.pk, pk_heads = pc.pk_heads, pkd = pc.pkd, nv4 = pc.nv4, w16 = pc.w16, gsplit = pc.gsplit;
    const int s_o = pc.s_o, s_d = pc.s_d, s_qkv_ws = pc.s_qkv, s_qkv = pc.s_qkv, s_gu = pc.s_gu, pk_so = pc.pk_so, pk_sd = pc.pk_sd, g_so = pc.g_so, g_sd = pc.g_sd;
    const int maxk = I > QD ? (I > H ? I : H) : (QD > H ? QD : H);
    const bool use_slabs = ws || g_so > 1 || g_sd > 1;
    const size_t slab_elems = std::max({(size_t)std::max({s_o, s_d, g_so, g_sd, pk_so, pk_sd}) * n * H, s_qkv > 1 ? (size_t)s_qkv * n * NQKV : 0,
                                        s_gu > 1 ? (size_t)s_gu * n * 2 * I : 0});
    // workspace: h32 [n,H] f32 | x [n,H] | qkv [n,NQKV] | attn [n,QD] | gu [n,2I] | act [n,I]  (bf16) | the split-K slabs |
    // w8a8 only: fp8 activations [n][maxk] + their scales [n][maxk/128], twice (the gate / up GEMM's SwiGLU epilogue writes the
    // second pair while q8 is its operand).  Run on a null base for the size, on the allocation for the pointers.
    float *h32, *slabs, *q8s, *q8bs;
    bf16 *x, *qkv, *attn, *gu, *act;
    uint8_t *q8, *q8b;
    auto layout = [&](void* base) -> size_t {
        uintptr_t p = (uintptr_t)base;
        const size_t rows = n;
        const bool pairs = c.weight_format == 2;
        size_t bytes = 512 + (pairs ? 2 * 512 : 0);   // slack for the roundings
        auto take = [&](auto*& dst, size_t b, bool held = true) { dst = (std::remove_reference_t<decltype(dst)>)p; p += b; if (held) bytes += b; };
        auto round256 = [&] { p = (p + 255) & ~(uintptr_t)255; };
        take(h32, rows * H * 4); take(x, rows * H * 2); take(qkv, rows * NQKV * 2); take(attn, rows * QD * 2); take(gu, rows * 2 * I * 2); take(act, rows * I * 2);
        round256(); take(slabs, use_slabs ? slab_elems * 4 : 0);
        round256(); take(q8, rows * maxk, pairs); take(q8s, rows * (maxk / 128) * 4, pairs);
        round256(); take(q8b, rows * maxk, pairs); take(q8bs, rows * (maxk / 128) * 4, pairs);
        return bytes;
    };
    const size_t need = layout(nullptr);
    if (need > e->pf_bytes) {
        if (e->pf) PGK_CHECK_HIP(hipStreamSynchronize(st));
        if (e->pf) pgk_free(e->pf);
        e->pf = nullptr;
        if (pgk_status r = pgk_malloc(&e->pf, need)) return r;
        e->pf_bytes = need;
    }
    const bool ids_by_value = n <= EMBED_ARG_TOKENS;   // the embedding kernel is the ids' only reader: short prompts pass them as arguments
    if (!ids_by_value && n > e->pf_tokens_cap) {
        if (e->pf_tokens) { PGK_CHECK_HIP(hipStreamSynchronize(st)); pgk_free(e->pf_tokens); }
        if (pgk_status r = pgk_malloc((void**)&e->pf_tokens, (size_t)n * 4)) return r;
        e->pf_tokens_cap = n;
    }
    for (int i = 0; i < n; ++i)
        PGK_REQUIRE(h_tokens[i] >= 0 && h_tokens[i] < c.vocab_size, "pgk_engine_prefill: token %d out of range", h_tokens[i]);
    if (!ids_by_value) {
        PGK_CHECK_HIP(hipMemcpyAsync(e->pf_tokens, h_tokens, (size_t)n * 4, hipMemcpyHostToDevice, st));
        PGK_CHECK_HIP(hipStreamSynchronize(st));  // h_tokens may be pageable: make the copy complete before returning control
    }
    const bool fp8 = pc.fp8, fp8act = pc.fp8act;
    layout(e->pf);
    int pending = 0;   // split-K slabs of the previous projection still to be added into h32 by the next norm
    // fp8act: RMSNorm and SwiGLU leave their result in q8/q8s themselves (x_in == nullptr); attention output is
    // quantised here (its rows span all heads, a flash workgroup only sees one)
    const bool fuse_q = pc.fuse_q, fuse_sw8 = pc.fuse_sw8, fuse_sw16 = pc.fuse_sw16, fuse_heads8 = pc.fuse_heads8, fuse_heads = pc.fuse_heads;
    // one projection: accum = h32 += x W^T (fp32), else dst = x W^T (bf16).  With splits > 1 the result is left as fp32
    // split-K slabs - accum: for the next norm to add into h32 (pending), else for the consumer kernel to sum
    auto proj = [&](const bf16* x_in, const void* w, const void* sc, void* dst, bool accum, int N_, int K_, int splits, const bf16* wp = nullptr) -> pgk_status {
        if (fp8act) {
            if (x_in)
                if (pgk_status r = quantize_fp8_rows_bf16(x_in, q8, q8s, n, K_, st)) return r;
            return gemm_fp8_nt(q8, q8s, (const uint8_t*)w, (const bf16*)sc, dst, accum, n, N_, K_, st);
        }
        if (!ws) {
            const bool usep = pkd && wp != nullptr;
            const int gs = accum && gsplit ? engine_gemm_pick_splits(n, N_, K_) : 1;
            if (gs > 1) { pending = gs; return engine_gemm_nt_slabs(x_in, usep ? (const void*)wp : w, slabs, gs, n, N_, K_, st, usep); }
            if (usep) return engine_gemm_nt(x_in, wp, nullptr, false, dst, accum, n, N_, K_, st, true);
            return engine_gemm_nt(x_in, w, (const bf16*)sc, fp8, dst, accum, n, N_, K_, st);
        }
        if (splits == 1) return wsgemm_nt(x_in, K_, w, (const bf16*)sc, fp8, dst, nullptr, accum ? 2 : 0, 1, n, N_, K_, st);   // wsgemm_pick_splits: >= 1
        if (accum) pending = splits;
        return wsgemm_nt(x_in, K_, w, (const bf16*)sc, fp8, slabs, nullptr, 1, splits, n, N_, K_, st);
    };
    auto norm = [&](const bf16* gamma, bool to_fp8 = false) -> pgk_status {
        return rmsnorm_slabs(h32, gamma, x, n, H, c.norm_eps, slabs, &pending, to_fp8 ? q8 : nullptr, to_fp8 ? q8s : nullptr, st, nullptr);
    };
    if (ids_by_value) {
        EmbedTokenArgs ids{};
        for (int i = 0; i < n; ++i) ids.id[i] = h_tokens[i];
        embed_rows_arg_kernel<<<n, 256, 0, st>>>(e->embed, h32, H, ids);
    } else {
        embed_rows_kernel<<<n, 256, 0, st>>>(e->embed, e->pf_tokens, h32, H);
    }
    PGK_LAUNCH_CHECK();
    const int kv_len = start_pos + n;
    int ss_n = 0;    // partial sums per row in pk_ss (carried norms)
    for (int l = 0; l < c.num_layers; ++l) {
        pgk_layer_weights_t Lq = e->layers[l];
        if (nv4) {
            // this layer's codes x scales -> bf16 [qkv | o | gate_up | down] in e->nv_deq (exact), read by the projections below
            bf16* d = e->nv_deq;
            const struct { const void* w; const void* s; int N, K; } m4[4] = {
                {Lq.w_qkv, Lq.s_qkv, NQKV, H}, {Lq.w_o, Lq.s_o, H, QD}, {Lq.w_gate_up, Lq.s_gate_up, 2 * I, H}, {Lq.w_down, Lq.s_down, H, I}};
            const void** dst[4] = {&Lq.w_qkv, &Lq.w_o, &Lq.w_gate_up, &Lq.w_down};
            for (int i = 0; i < 4; ++i) {
                if (pgk_status r = dequant_nvf4_nk((const uint8_t*)m4[i].w, (const uint8_t*)m4[i].s, d, m4[i].N, m4[i].K, st)) return r;
                *dst[i] = d;
                d += (size_t)m4[i].N * m4[i].K;
            }
            Lq.s_qkv = Lq.s_o = Lq.s_gate_up = Lq.s_down = nullptr;
        }
        const auto& L = Lq;
        bf16* kc = e->kcache + (size_t)l * e->kv_layer_elems() + (size_t)seq * c.num_kv_heads * c.max_seq_len * D;
        bf16* vc = e->vcache + (size_t)l * e->kv_layer_elems() + (size_t)seq * c.num_kv_heads * c.max_seq_len * D;
        // packed path with carried norms: layer 0 normalises with a launch; afterwards x holds bf16(h * gamma) and pk_ss the
        // row statistics, both left by the previous layer's down_proj
        const bool carried = pc.carried;
        PkArgs nrm{};                                   // how the consumer of x scales its rows (all null: x is normalised)
        if (carried && l > 0) { nrm.ss_in = e->pk_ss; nrm.ss_n = ss_n; nrm.ss_eps = c.norm_eps; }
        else if (pgk_status r = norm((const bf16*)L.attn_norm, fuse_q)) return r;
        if (pk_heads) {
            PkArgs hd = nrm;
            fill_head_args(hd, e, L, kc, vc, start_pos);
            if (pgk_status r = pkgemm_nt(x, H, e->packed[l].qkv, qkv, NQKV, PK_EPI_QKV, 1, n, NQKV, H, &hd, st)) return r;
        } else if (pk) {
            if (pgk_status r = pkgemm_nt(x, H, e->packed[l].qkv, qkv, NQKV, PK_EPI_BF16, 1, n, NQKV, H, &nrm, st)) return r;
        } else if (fuse_heads) {
            QkvHeadArgs hd{};
            fill_head_args(hd, e, L, kc, vc, start_pos);
            if (fuse_heads8) {
                if (pgk_status r = gemm_fp8_qkv_heads_nt(q8, q8s, (const uint8_t*)L.w_qkv, (const bf16*)L.s_qkv, qkv, n, NQKV, H, hd, st)) return r;
            } else if (pgk_status r = engine_gemm_qkv_heads_nt(x, pkd ? e->packed[l].qkv : (const bf16*)L.w_qkv, qkv, n, NQKV, H, hd, st, pkd)) return r;
        } else {
            if (pgk_status r = proj(fuse_q ? nullptr : x, L.w_qkv, L.s_qkv, qkv, false, NQKV, H, s_qkv, pkd ? e->packed[l].qkv : nullptr)) return r;
        }
        if (!pk_heads && !fuse_heads) {
            const int s_qkv = pk ? 1 : s_qkv_ws;
            const int nslots = c.num_heads + 2 * c.num_kv_heads;
            const bf16* qg = c.use_qk_norm ? (const bf16*)L.q_norm : nullptr;
            const bf16* kg = c.use_qk_norm ? (const bf16*)L.k_norm : nullptr;
            const auto kfn = D == 128 ? qknorm_rope_kvwrite_kernel<128> : qknorm_rope_kvwrite_kernel<64>;
            kfn<<<ceil_div((long long)n * nslots, D == 128 ? 16 : 32), 256, 0, st>>>(
                qkv, qg, kg, c.norm_eps, e->rope_cos, e->rope_sin, kc, vc, n, c.num_heads, c.num_kv_heads, c.max_seq_len, start_pos, slabs,
                s_qkv > 1 ? s_qkv : 0);
            PGK_LAUNCH_CHECK();
        }
        // fp8 x fp8: a head's 128 output dims are one scale block of the o_proj operand, so the flash kernel quantises them itself
        const bool attn_q8 = fuse_q && D == 128 && n > 128 && sdpa_flash_enabled();
        if (attn_q8) {
            if (pgk_status r = flash_prefill_q8(qkv, kc, vc, q8, q8s, c.num_heads, c.num_kv_heads, n, kv_len, 1.0f / sqrtf((float)D), D, NQKV,
                                                (long long)c.max_seq_len * D, D, st))
                return r;
        } else if (pgk_status r = pgk_sdpa_causal(qkv, kc, vc, attn, c.num_heads, c.num_kv_heads, n, kv_len, D, 0.f, D, NQKV,
                                                  (int64_t)c.max_seq_len * D, D, D, QD, PGK_BF16, st))
            return r;
        // N = hidden projections of the packed path: fp32 split-K slabs summed by the next norm (or h32 += with one split)
        auto pk_accum = [&](const bf16* x_in, const bf16* wp, int K_, int splits) -> pgk_status {
            if (splits == 1) return pkgemm_nt(x_in, K_, wp, h32, H, PK_EPI_ACCUM, 1, n, H, K_, nullptr, st);
            pending = splits;
            return pkgemm_nt(x_in, K_, wp, slabs, H, PK_EPI_SLAB, splits, n, H, K_, nullptr, st);
        };
        if (carried) {
            if (pgk_status r = packed_mlp_carried(e, l, n, attn, act, h32, x, &ss_n, st, nullptr)) return r;
            continue;
        }
        if (pk) { if (pgk_status r = pk_accum(attn, e->packed[l].o, QD, pk_so)) return r; }
        else if (pgk_status r = proj(attn_q8 ? nullptr : attn, L.w_o, L.s_o, h32, true, H, QD, s_o, pkd ? e->packed[l].o : nullptr)) return r;
        if (pgk_status r = norm((const bf16*)L.mlp_norm, fuse_q)) return r;
        if (pk) {
            // SwiGLU inside the gate_up projection: the gate tile and its up tile live in the same wave
            if (pgk_status r = pkgemm_nt(x, H, e->packed[l].gate_up, act, I, PK_EPI_SWIGLU, 1, n, 2 * I, H, nullptr, st)) return r;
            if (pgk_status r = pk_accum(act, e->packed[l].down, I, pk_sd)) return r;
            continue;
        }
        if (fuse_sw8) {
            // x's codes in q8 -> act's codes in q8b; the down projection reads q8b
            if (pgk_status r = gemm_fp8_swiglu_nt(q8, q8s, (const uint8_t*)L.w_gate_up, (const bf16*)L.s_gate_up, q8b, q8bs, n, I, H, st)) return r;
            if (pgk_status r = gemm_fp8_nt(q8b, q8bs, (const uint8_t*)L.w_down, (const bf16*)L.s_down, h32, true, n, H, I, st)) return r;
            continue;
        }
        if (fuse_sw16) {
            if (pgk_status r = engine_gemm_swiglu_nt(x, pkd ? (const void*)e->packed[l].gate_up : L.w_gate_up, (const bf16*)L.s_gate_up, fp8 && !pkd, act, n, I, H, st, pkd)) return r;
            if (pgk_status r = proj(act, L.w_down, L.s_down, h32, true, H, I, s_d, pkd ? e->packed[l].down : nullptr)) return r;
            continue;
        }
        if (pgk_status r = proj(fuse_q ? nullptr : x, L.w_gate_up, L.s_gate_up, gu, false, 2 * I, H, s_gu, pkd ? e->packed[l].gate_up : nullptr)) return r;
        swiglu_rows_kernel<<<ceil_div((long long)n * I / 8, 256) > 2048 ? 2048 : ceil_div((long long)n * I / 8, 256), 256, 0, st>>>(
            gu, act, n, I, slabs, s_gu > 1 ? s_gu : 0, fuse_q ? q8 : nullptr, fuse_q ? q8s : nullptr);
        PGK_LAUNCH_CHECK();
        if (pgk_status r = proj(fuse_q ? nullptr : act, L.w_down, L.s_down, h32, true, H, I, s_d, pkd ? e->packed[l].down : nullptr)) return r;
    }
    if (pgk_status r = norm(e->final_norm)) return r;
    if (all_logits) {
        if (pgk_status r = engine_gemm_nt(x, e->lm_head, nullptr, false, all_logits, false, n, c.vocab_size, H, st)) return r;
    }
    if (h_last_logits) {
        // last row through the fp32-output GEMV (the decode lm_head kernel with a plain prologue)
        float* xin = h32;  // reuse: widen the last normed row
        bf16_rows_to_f32_kernel<<<4, 256, 0, st>>>(x + (size_t)(n - 1) * H, xin, H);
        PGK_LAUNCH_CHECK();
        FusedArgs a{};
        a.w = e->lm_head; a.N = c.vocab_size; a.K = H; a.xin = xin;
        a.out = e->logits + (size_t)seq * c.vocab_size; a.ld_out = c.vocab_size;
        if (pgk_status r = launch_fused<bf16, float, 1, 4, PRO_PLAIN, EPI_STORE>(a, c.vocab_size, st)) return r;
        PGK_CHECK_HIP(hipMemcpyAsync(h_last_logits, a.out, (size_t)c.vocab_size * 4, hipMemcpyDeviceToHost, st));
        PGK_CHECK_HIP(hipStreamSynchronize(st));
    }
    return PGK_OK;
}

}  // extern "C"
