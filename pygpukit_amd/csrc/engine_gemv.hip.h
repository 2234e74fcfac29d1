// Fused GEMV decode kernel (prologue builds x[M][K] in LDS, body streams W, epilogue consumes y) and its launchers.
#pragma once

#include <type_traits>

#include "engine_common.hip.h"
#include "engine_state.hip.h"

namespace pgk {

template <class XT> __device__ __forceinline__ void store_x(XT* xs, int i, float v);
template <> __device__ __forceinline__ void store_x<float>(float* xs, int i, float v) { xs[i] = v; }
template <> __device__ __forceinline__ void store_x<bf16>(bf16* xs, int i, float v) { xs[i] = from_f<bf16>(v); }

// C = number of 16-byte chunks per weight row held per lane.  C > 0 fixes K = C * 64 * NW at COMPILE
// time: the whole row set of the wave's first trip is preloaded before the prologue touches the
// activations, and every prologue loop has an exact trip count - straight-line code, no guarded loads.
// (A load under a per-lane guard, or accumulated inside a conditional, is waited for on the spot by
// hipcc: that serialised dozens of memory round trips per kernel in the first version.)  C == 0 is the
// generic any-K path.
template <class WT, class XT, int M, int R, int PRO, int EPI, int C>
__global__ __launch_bounds__(256) void fused_gemv_kernel(unsigned long long* tl, const void* w_, const bf16* wscale_, const float* x_, const bf16* gamma_,
                                                         const float* aux_, int N_, int naux_, FusedArgs a) {
    // The first 14 dwords of the kernel arguments - everything the load-issue phase needs - arrive PRELOADED in SGPRs
    // (-mllvm -amdgpu-kernarg-preload-count=14, see the Makefile): x_ = the fp32 input rows (FusedArgs::h for the norm
    // prologues, FusedArgs::xin for PRO_PLAIN), aux_ / naux_ = the o_proj partial vectors and their count (PRO_NORM_SUM) or the residual rows and
    // their leading dimension (EPI_RESID).  What is left in the by-value struct (eps, out, ld_out, h_out, argmax slots) is
    // fetched by scalar loads that complete under the weight stream.  Before, every load of the kernel waited for the
    // struct's s_load through a scalar cache the dispatch had just invalidated.
    static_assert(!(PRO == PRO_NORM_SUM && EPI == EPI_RESID), "aux_ cannot carry partial vectors and residual rows at once");
    const TLStamp tls(tl);
    constexpr int NW = WTraits<WT>::NW;
    constexpr bool FP8 = std::is_same<WT, fp8e4m3>::value;
    constexpr bool NV4 = std::is_same<WT, nvf4x2>::value;   // wscale_ then holds the uint8 scale bytes [N, K/32]
    // NVF4: C counts 1024-k units (32 lanes x 32 k); an odd C leaves the upper half-wave of the last chunk without a k of
    // its own - it re-reads the lower half's and weighs it 0
    constexpr int KC = NV4 ? C * 1024 : C * 64 * NW;   // compile-time K (0 = runtime)
    constexpr int CL = NV4 ? (C + 1) / 2 : C;          // 16-byte chunks per lane and row
    constexpr int KJ = KC / 256;              // activation elements per thread
    extern __shared__ __attribute__((aligned(16))) char smem[];
    XT* xs = reinterpret_cast<XT*>(smem);  // [M][K]
    __shared__ float red[16];
    __shared__ float s_bv[4][M];
    __shared__ int s_bi[4][M];
    const int K = (C > 0) ? KC : a.K;
    const int N = N_;
    // wid through readfirstlane: the wave's rows, their base addresses and the trip loop's branches are then scalar
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int OUT_PER_TRIP = (EPI == EPI_SWIGLU) ? R / 2 : R;
    const int wave = blockIdx.x * 4 + wid, nwaves = gridDim.x * 4;
    // The epilogue is lane-parallel: output (r, m) of a trip - row n0 + r of sequence m - belongs to lane m * OUT_PER_TRIP + r.
    constexpr int NOUT = OUT_PER_TRIP * M;
    static_assert(NOUT <= 64, "a trip's outputs fit the lanes of a wave");
    const int my_m = min(lane, NOUT - 1) / OUT_PER_TRIP, my_r = min(lane, NOUT - 1) - my_m * OUT_PER_TRIP;

    auto row_of = [&](int n0, int r) -> int {
        if constexpr (EPI == EPI_SWIGLU) return (r < R / 2) ? min(n0 + r, N - 1) : N + min(n0 + r - R / 2, N - 1);
        else return min(n0 + r, N - 1);
    };

    constexpr int CLD = CL > 0 ? CL : 1;
    uint4 pre[R][CLD];
    uint32_t psc[R][CLD];   // the scales as loaded (fp8: bf16 bits of the block scale; NVF4: the scale byte), converted where consumed
    float resv = 0.f;
    // every global load of one trip (C > 0): the R rows from output nfirst on (clamped), scales alongside the weights.  Nothing
    // here touches a loaded value: a conversion at this point would be waited for inside the issue block.
    auto load_trip = [&](uint4 (&wq)[R][CLD], uint32_t (&sq)[R][CLD], int nfirst) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int row = row_of(nfirst, r);
            if constexpr (NV4) {
                const uint8_t* wr = reinterpret_cast<const uint8_t*>(w_) + (size_t)row * (KC >> 1);
                const uint8_t* sr = reinterpret_cast<const uint8_t*>(wscale_) + (size_t)row * (KC >> 5);
#pragma unroll
                for (int c = 0; c < CL; ++c) {
                    const int k0 = lane * NW + c * 64 * NW, kk = k0 < KC ? k0 : k0 - 1024;
                    wq[r][c] = load_nt16(wr + (kk >> 1));
                    sq[r][c] = sr[kk >> 5];
                }
                continue;
            }
            const WT* wr = reinterpret_cast<const WT*>(w_) + (size_t)row * KC;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int k0 = lane * NW + c * 64 * NW;
                wq[r][c] = load_nt16(wr + k0);
                if constexpr (FP8) sq[r][c] = wscale_[(size_t)(row >> 7) * (KC >> 7) + (k0 >> 7)].bits;
            }
        }
    };
    if constexpr (C > 0) {
        // ---- all global loads of the first trip, issued back to back; nothing is waited for until the prologue's ALU ----
        // Vector memory returns in ISSUE order.  The activation vectors are a few KB that the previous kernel left in L2,
        // the weight rows come from HBM: issued first, the activations are usable ~1 us before the weights land and the
        // whole prologue (norm statistic, barrier, LDS image) runs under the weight latency.  (The first version issued
        // the weights first: the prologue then started only after the last weight chunk had arrived - in-kernel stamps,
        // tools/phase_stamps.py.)
        const int nf = min(wave * OUT_PER_TRIP, N - 1);  // waves beyond N recompute the last rows (never stored)
        constexpr bool NORM = PRO == PRO_NORM || PRO == PRO_NORM_SUM;
        constexpr int NP = (PRO == PRO_NORM_SUM) ? 8 : 1;
        const int np = (PRO == PRO_NORM_SUM) ? naux_ : 1;
        float hv[M][KJ], gv[NORM ? KJ : 1], pvs[PRO == PRO_NORM_SUM ? M : 1][PRO == PRO_NORM_SUM ? KJ : 1][NP];
        // A thread owns KJ / VW runs of VW consecutive elements (run v starts at element (256 v + thread) * VW): every load of
        // the prologue is one 16-byte (K % 1024 == 0) or 8-byte access per run - a quarter of the instructions of the
        // element-per-load form, and the texture addresser moves 1 KiB instead of 256 B per wave-instruction.  The gate/up
        // kernel reads nine such vectors (h + 8 o_proj partials) in every workgroup: more bytes through a CU's addresser
        // than its share of the weights.
        constexpr int VW = (KJ % 4 == 0) ? 4 : 2, NV = KJ / VW;
        auto run0 = [&](int v) -> int { return (256 * v + (int)threadIdx.x) * VW; };
        auto ldrun = [&](const float* base, int v, float* dst) {
            if constexpr (VW == 4) { const float4 t = *reinterpret_cast<const float4*>(base + run0(v)); dst[0] = t.x; dst[1] = t.y; dst[2] = t.z; dst[3] = t.w; }
            else { const float2 t = *reinterpret_cast<const float2*>(base + run0(v)); dst[0] = t.x; dst[1] = t.y; }
        };
        auto strun = [&](float* base, int v, const float* src) {
            if constexpr (VW == 4) *reinterpret_cast<float4*>(base + run0(v)) = make_float4(src[0], src[1], src[2], src[3]);
            else *reinterpret_cast<float2*>(base + run0(v)) = make_float2(src[0], src[1]);
        };
        auto stx = [&](int m, int v, const float* src) {        // the LDS image of row m (NVF4: swizzled, a run stays in one group)
            const int at = NV4 ? nvf4_xpos<XT>(run0(v), KC) : run0(v);
            if constexpr (std::is_same<XT, float>::value) {
                float* d = reinterpret_cast<float*>(xs) + (size_t)m * KC + at;
                if constexpr (VW == 4) *reinterpret_cast<float4*>(d) = make_float4(src[0], src[1], src[2], src[3]);
                else *reinterpret_cast<float2*>(d) = make_float2(src[0], src[1]);
            }
            else if constexpr (VW == 4) *reinterpret_cast<uint2*>(xs + (size_t)m * KC + at) = make_uint2(pack_bf16x2(src[0], src[1]), pack_bf16x2(src[2], src[3]));
            else *reinterpret_cast<uint32_t*>(xs + (size_t)m * KC + at) = pack_bf16x2(src[0], src[1]);
        };
        // ---- activation loads ----
        // the residual word of the first trip, loaded by the lane that adds it (lanes past NOUT re-read the last one)
        if constexpr (EPI == EPI_RESID) resv = *(aux_ + (size_t)my_m * naux_ + min(nf + my_r, N - 1));
        if constexpr (NORM) {
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                if constexpr (VW == 4) {
                    const uint2 g = *reinterpret_cast<const uint2*>(gamma_ + run0(v));
                    gv[4 * v] = __uint_as_float(g.x << 16); gv[4 * v + 1] = __uint_as_float(g.x & 0xFFFF0000u);
                    gv[4 * v + 2] = __uint_as_float(g.y << 16); gv[4 * v + 3] = __uint_as_float(g.y & 0xFFFF0000u);
                } else {
                    const uint32_t g = *reinterpret_cast<const uint32_t*>(gamma_ + run0(v));
                    gv[2 * v] = __uint_as_float(g << 16); gv[2 * v + 1] = __uint_as_float(g & 0xFFFF0000u);
                }
#pragma unroll
                for (int m = 0; m < M; ++m) ldrun(x_ + (size_t)m * KC, v, &hv[m][VW * v]);
            }
            if constexpr (PRO == PRO_NORM_SUM) {
                // partial vectors: unconditional clamped loads, masked adds below (one round trip for up to 8)
#pragma unroll
                for (int m = 0; m < M; ++m)
#pragma unroll
                    for (int p = 0; p < NP; ++p)
#pragma unroll
                        for (int v = 0; v < NV; ++v) {
                            float t[VW];
                            ldrun(aux_ + ((size_t)m * np + min(p, np - 1)) * KC, v, t);
#pragma unroll
                            for (int e = 0; e < VW; ++e) pvs[m][VW * v + e][p] = t[e];
                        }
            }
        } else if constexpr (PRO == PRO_PLAIN) {
#pragma unroll
            for (int m = 0; m < M; ++m)
#pragma unroll
                for (int v = 0; v < NV; ++v) ldrun(x_ + (size_t)m * KC, v, &hv[m][VW * v]);
        }
        __builtin_amdgcn_sched_barrier(0);      // keep the compiler from hoisting the weight stream above the small loads
        load_trip(pre, psc, nf);
        __builtin_amdgcn_sched_barrier(0);
        // ---- prologue ALU, exact trip counts ----
        if constexpr (NORM) {
            if constexpr (PRO == PRO_NORM_SUM) {
#pragma unroll
                for (int m = 0; m < M; ++m)
#pragma unroll
                    for (int j = 0; j < KJ; ++j)
#pragma unroll
                        for (int p = 0; p < NP; ++p) hv[m][j] += (p < np) ? pvs[m][j][p] : 0.f;
                // more than NP partial vectors (models with more than 8 kv heads): the rest in a second trip.  (Until this loop
                // existed partials 8.. were silently dropped: batch-1 / batch-2 decode of a 16-kv-head model was wrong.)
                for (int p = NP; p < np; ++p)
#pragma unroll
                    for (int m = 0; m < M; ++m)
#pragma unroll
                        for (int v = 0; v < NV; ++v) {
                            float t[VW];
                            ldrun(aux_ + ((size_t)m * np + p) * KC, v, t);
#pragma unroll
                            for (int e = 0; e < VW; ++e) hv[m][VW * v + e] += t[e];
                        }
            }
            float ss[M];
#pragma unroll
            for (int m = 0; m < M; ++m) {
                ss[m] = 0.f;
#pragma unroll
                for (int j = 0; j < KJ; ++j) ss[m] = fmaf(hv[m][j], hv[m][j], ss[m]);
                ss[m] = wave_sum(ss[m]);
            }
            if (lane == 0) {
#pragma unroll
                for (int m = 0; m < M; ++m) s_bv[wid][m] = ss[m];
            }
            __syncthreads();
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const float tot = s_bv[0][m] + s_bv[1][m] + s_bv[2][m] + s_bv[3][m];
                const float inv = 1.0f / sqrtf(tot / KC + a.eps);
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    if constexpr (PRO == PRO_NORM_SUM) { if (blockIdx.x == 0) strun(a.h_out + (size_t)m * KC, v, &hv[m][VW * v]); }
                    float t[VW];
#pragma unroll
                    for (int e = 0; e < VW; ++e) t[e] = hv[m][VW * v + e] * inv * gv[VW * v + e];
                    stx(m, v, t);
                }
            }
        } else if constexpr (PRO == PRO_PLAIN) {
#pragma unroll
            for (int m = 0; m < M; ++m)
#pragma unroll
                for (int v = 0; v < NV; ++v) stx(m, v, &hv[m][VW * v]);
        }
    }
    if constexpr (C == 0) {
        // ---- generic prologue (any K) ----
        if constexpr (PRO == PRO_NORM || PRO == PRO_NORM_SUM) {
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const float* hr = x_ + (size_t)m * K;
                auto xin = [&](int i) -> float {
                    float v = hr[i];
                    if constexpr (PRO == PRO_NORM_SUM) {
                        for (int p = 0; p < naux_; ++p) v += aux_[((size_t)m * naux_ + p) * K + i];
                    }
                    return v;
                };
                float ss = 0.f;
                for (int i = threadIdx.x; i < K; i += 256) { const float v = xin(i); ss = fmaf(v, v, ss); }
                ss = block_sum(ss, red);
                const float inv = 1.0f / sqrtf(ss / K + a.eps);
                for (int i = threadIdx.x; i < K; i += 256) {
                    const float v = xin(i);
                    if constexpr (PRO == PRO_NORM_SUM) { if (blockIdx.x == 0) a.h_out[(size_t)m * K + i] = v; }
                    store_x<XT>(xs, m * K + (NV4 ? nvf4_xpos<XT>(i, K) : i), v * inv * to_f(gamma_[i]));
                }
            }
        } else if constexpr (PRO == PRO_PLAIN) {
            if constexpr (NV4) {
#pragma unroll
                for (int m = 0; m < M; ++m)
                    for (int i = threadIdx.x; i < K; i += 256) store_x<XT>(xs, m * K + nvf4_xpos<XT>(i, K), x_[(size_t)m * K + i]);
            } else {
                for (int i = threadIdx.x; i < M * K; i += 256) store_x<XT>(xs, i, x_[i]);
            }
        }
    }
    __syncthreads();

    // ---- body ----
    // EPI_LOGITS: every lane's running best over its OWN outputs (rows ascend from trip to trip, so `>` keeps the lowest row)
    float best_v = -INFINITY;
    int best_i = 0x7FFFFFFF;

    // one trip's chunks, held in registers (C > 0), against the LDS image: row by row chunk 0 .. CL - 1, elements in order
    auto consume = [&](const uint4 (&wq)[R][CLD], const uint32_t (&sq)[R][CLD], float (&acc)[R][M]) {
#pragma unroll
        for (int c = 0; c < CLD; ++c) {
            const int k0 = lane * NW + c * 64 * NW;
            if constexpr (std::is_same<WT, bf16>::value && std::is_same<XT, bf16>::value) {
                uint4 xr[M];
#pragma unroll
                for (int m = 0; m < M; ++m) xr[m] = *reinterpret_cast<const uint4*>(xs + (size_t)m * K + k0);
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int m = 0; m < M; ++m) acc[r][m] = dot8_bf16(wq[r][c], xr[m], acc[r][m]);
            } else if constexpr (NV4) {
                uint4 raw[R];
                float p[R][M];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    raw[r] = wq[r][c];
#pragma unroll
                    for (int m = 0; m < M; ++m) p[r][m] = 0.f;
                }
                nvf4_dot32<XT, M, R>(raw, xs, K, k0 < KC ? k0 : k0 - 1024, p);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float sc = k0 < KC ? nvf4_scale_value(sq[r][c]) : 0.f;
#pragma unroll
                    for (int m = 0; m < M; ++m) acc[r][m] = fmaf(sc, p[r][m], acc[r][m]);
                }
            } else {
                float xf[M][NW];
#pragma unroll
                for (int m = 0; m < M; ++m) XLoad<XT, NW>::load(xs + (size_t)m * K + k0, xf[m]);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    float wf[NW];
                    WTraits<WT>::decode(wq[r][c], wf);
#pragma unroll
                    for (int m = 0; m < M; ++m) {
                        if constexpr (FP8) {
                            float p = 0.f;
#pragma unroll
                            for (int j = 0; j < NW; ++j) p = fmaf(wf[j], xf[m][j], p);
                            acc[r][m] = fmaf(bf16_bits_to_f((uint16_t)sq[r][c]), p, acc[r][m]);
                        } else {
#pragma unroll
                            for (int j = 0; j < NW; ++j) acc[r][m] = fmaf(wf[j], xf[m][j], acc[r][m]);
                        }
                    }
                }
            }
        }
    };
    // one trip streamed from memory as it is consumed: every trip of the any-K path (C == 0), the later trips otherwise
    auto stream_trip = [&](int n0, float (&acc)[R][M]) {
        if constexpr (NV4) {
            const uint8_t* wrow[R];
            const uint8_t* srow[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int row = row_of(n0, r);
                wrow[r] = reinterpret_cast<const uint8_t*>(w_) + (size_t)row * (K >> 1);
                srow[r] = reinterpret_cast<const uint8_t*>(wscale_) + (size_t)row * (K >> 5);
            }
            gemv_rows_nvf4<XT, M, R>(wrow, srow, xs, K, K, lane, acc);
        } else {
            const WT* wrow[R];
            const bf16* srow[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int row = row_of(n0, r);
                wrow[r] = reinterpret_cast<const WT*>(w_) + (size_t)row * K;
                srow[r] = wscale_ ? wscale_ + (size_t)(row >> 7) * (K >> 7) : nullptr;
            }
            if constexpr (FP8) gemv_rows_fp8<XT, M, R>(wrow, srow, xs, K, K, lane, acc);
            else gemv_rows<WT, XT, M, R>(wrow, xs, K, K, lane, acc);
        }
    };
    // ---- the tail of a trip: R * M wave sums side by side, then ONE epilogue across the lanes ----
    // Lane m * OUT_PER_TRIP + r picks output (r, m) out of the wave-uniform sums, so the SwiGLU (one exp, one IEEE division),
    // the residual add and the store are each a single instruction sequence and one predicated store to consecutive
    // addresses per sequence.  (Before: lane 0 alone walked the outputs, each behind its own branch - three copies of the
    // 24-instruction SwiGLU in a row in the gate/up kernel - after R * M reductions run one after the other.)
    auto tail = [&](int n0, float (&acc)[R][M], bool have_res, float res) {
        float s[R * M];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int m = 0; m < M; ++m) s[r * M + m] = acc[r][m];
        wave_sum_n<R * M>(s);
        float val = s[0], up = s[(R / 2) * M];
#pragma unroll
        for (int m = 0; m < M; ++m)
#pragma unroll
            for (int r = 0; r < OUT_PER_TRIP; ++r) {
                const bool mine = lane == m * OUT_PER_TRIP + r;
                val = mine ? s[r * M + m] : val;
                if constexpr (EPI == EPI_SWIGLU) up = mine ? s[(r + R / 2) * M + m] : up;
            }
        if constexpr (EPI == EPI_SWIGLU) val = silu_mul(val, up);
        if (lane < NOUT && n0 + my_r < N) {
            const size_t o = (size_t)my_m * a.ld_out + n0 + my_r;
            if constexpr (EPI == EPI_RESID) {
                const float base = have_res ? res : *(aux_ + o);   // the any-K path loads it here
                *(a.out + o) = base + val;
            } else {
                *(a.out + o) = val;                  // EPI_LOGITS: read by later launches only, ordinary stores
            }
            if constexpr (EPI == EPI_LOGITS) {
                if (val > best_v) { best_v = val; best_i = n0 + my_r; }
            }
        }
    };
    auto clear = [](float (&acc)[R][M]) {
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int m = 0; m < M; ++m) acc[r][m] = 0.f;
    };

    // The preloaded first trip stands in front of the loop, so its registers die there; every later trip (the lm_head makes
    // nine or ten) and the whole any-K path stream their rows as they consume them.
    if constexpr (C > 0) {
        if (wave * OUT_PER_TRIP < N) {
            float acc[R][M];
            clear(acc);
            consume(pre, psc, acc);
#ifdef PGK_PHASE_STAMPS
            // the stamp's clock read depends on nothing: tie it to the sums, or it is placed in front of the FMAs and their waits
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int m = 0; m < M; ++m) asm volatile("" : "+v"(acc[r][m]));
#endif
            tls.phase(0);
            tail(wave * OUT_PER_TRIP, acc, true, resv);
            tls.phase(1);
        }
    }
    for (int g = wave + (C > 0 ? nwaves : 0); g * OUT_PER_TRIP < N; g += nwaves) {
        float acc[R][M];
        clear(acc);
        stream_trip(g * OUT_PER_TRIP, acc);
        tail(g * OUT_PER_TRIP, acc, false, 0.f);
    }
    if constexpr (EPI == EPI_LOGITS) {
        __syncthreads();  // s_bv may still be read by the prologue reduction of a slower wave
        // the lanes' bests merged once: greater value wins, lowest row on ties - what lane 0's walk over the rows gave
        float wv[M];
        int wi[M];
#pragma unroll
        for (int m = 0; m < M; ++m) {
            wv[m] = readlane_f(best_v, m * OUT_PER_TRIP);
            wi[m] = __builtin_amdgcn_readlane(best_i, m * OUT_PER_TRIP);
#pragma unroll
            for (int r = 1; r < OUT_PER_TRIP; ++r) {
                const float v = readlane_f(best_v, m * OUT_PER_TRIP + r);
                const int i = __builtin_amdgcn_readlane(best_i, m * OUT_PER_TRIP + r);
                if (v > wv[m] || (v == wv[m] && i < wi[m])) { wv[m] = v; wi[m] = i; }
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int m = 0; m < M; ++m) { s_bv[wid][m] = wv[m]; s_bi[wid][m] = wi[m]; }
        }
        __syncthreads();
        if (threadIdx.x < M) {
            const int m = threadIdx.x;
            float bv = s_bv[0][m];
            int bi = s_bi[0][m];
            for (int w = 1; w < 4; ++w)
                if (s_bv[w][m] > bv || (s_bv[w][m] == bv && s_bi[w][m] < bi)) { bv = s_bv[w][m]; bi = s_bi[w][m]; }
            a.amax_val[(size_t)m * gridDim.x + blockIdx.x] = bv;
            a.amax_idx[(size_t)m * gridDim.x + blockIdx.x] = bi;
        }
    }
    tls.end();
}

template <class WT, class XT, int M, int R, int PRO, int EPI, int C>
static pgk_status launch_fused_c(const FusedArgs& a, int n_out, hipStream_t st, int force_grid) {
    const size_t lds = (size_t)M * a.K * sizeof(XT);
    PGK_REQUIRE(lds <= 156 * 1024, "engine: %d activation rows of K=%d do not fit LDS", M, a.K);
    auto kfn = &fused_gemv_kernel<WT, XT, M, R, PRO, EPI, C>;
    static bool attr_done = false;
    if (lds > 48 * 1024 && !attr_done) {
        PGK_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 2048));
        attr_done = true;
    }
    const int grid = gemv_grid(R, EPI == EPI_SWIGLU, n_out, force_grid);   // engine_state.hip.h
    const float* x = (PRO == PRO_PLAIN) ? a.xin : a.h;
    const float* aux = (PRO == PRO_NORM_SUM) ? a.part : a.res;
    const int naux = (PRO == PRO_NORM_SUM) ? a.nsplit : a.ld_out;
    PGK_CHECK_HIP(launch_k(kfn, dim3(grid), dim3(256), lds, st, a.w, a.wscale, x, a.gamma, aux, a.N, naux, a));
    return PGK_OK;
}

// The preload depth C (gemv_preload, engine_state.hip.h): the row's chunks sit in registers when it is short enough.
template <class WT, class XT, int M, int R, int PRO, int EPI>
static pgk_status launch_fused(const FusedArgs& a, int n_out, hipStream_t st, int force_grid = 0) {
    constexpr bool NV4 = std::is_same<WT, nvf4x2>::value;   // NVF4: C in 1024-k units, (C + 1) / 2 chunks per lane
    const int c = gemv_preload(WTraits<WT>::NW, R, a.K);
    constexpr int BUDGET = 12 / R;  // R*C*4 preload VGPRs <= 48: the depths gemv_preload can return for this R are the ones instantiated
    if constexpr (1 <= BUDGET) { if (c == 1) return launch_fused_c<WT, XT, M, R, PRO, EPI, 1>(a, n_out, st, force_grid); }
    if constexpr ((NV4 ? 1 : 2) <= BUDGET) { if (c == 2) return launch_fused_c<WT, XT, M, R, PRO, EPI, 2>(a, n_out, st, force_grid); }
    if constexpr ((NV4 ? 2 : 3) <= BUDGET) { if (c == 3) return launch_fused_c<WT, XT, M, R, PRO, EPI, 3>(a, n_out, st, force_grid); }
    if constexpr ((NV4 ? 2 : 4) <= BUDGET) { if (c == 4) return launch_fused_c<WT, XT, M, R, PRO, EPI, 4>(a, n_out, st, force_grid); }
    if constexpr ((NV4 ? 3 : 6) <= BUDGET) { if (c == 6) return launch_fused_c<WT, XT, M, R, PRO, EPI, 6>(a, n_out, st, force_grid); }
    PGK_REQUIRE(c == 0, "engine: preload depth %d at %d rows per wave is not instantiated", c, R);
    return launch_fused_c<WT, XT, M, R, PRO, EPI, 0>(a, n_out, st, force_grid);
}

// The rows per wave R (gemv_rows, engine_state.hip.h); only the R a (weight kind, M, epilogue) can be given are instantiated.
template <class WT, class XT, int M, int PRO, int EPI>
static pgk_status launch_fused_auto(const FusedArgs& a, int n_out, hipStream_t st) {
    const int r = gemv_rows(WTraits<WT>::NW, M, EPI == EPI_SWIGLU, n_out, a.K);
    if constexpr (std::is_same<WT, nvf4x2>::value && M >= 4) {
        if (r == 2) return launch_fused<WT, XT, M, 2, PRO, EPI>(a, n_out, st);
    } else if constexpr (EPI == EPI_SWIGLU) {
        if constexpr (M == 1) { if (r == 6) return launch_fused<WT, XT, M, 6, PRO, EPI>(a, n_out, st); }
        if (r == 4) return launch_fused<WT, XT, M, 4, PRO, EPI>(a, n_out, st);
        if (r == 2) return launch_fused<WT, XT, M, 2, PRO, EPI>(a, n_out, st);
    } else {
        if (r == 4) return launch_fused<WT, XT, M, 4, PRO, EPI>(a, n_out, st);
        if (r == 2) return launch_fused<WT, XT, M, 2, PRO, EPI>(a, n_out, st);
        if (r == 1) return launch_fused<WT, XT, M, 1, PRO, EPI>(a, n_out, st);
    }
    return set_error(PGK_ERR_UNSUPPORTED, "engine: %d rows per wave are not instantiated for this projection", r);
}

}  // namespace pgk
