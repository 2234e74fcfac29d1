// The weight-streaming walk shared by the skinny dense GEMM (ops_wsgemm.hip) and the grouped expert GEMM's few-rows regime
// (ops_moe.hip):  acc[mt] += A[mt*16 .. +16][kbeg, kend) . W[n0 + wave's 16 rows][kbeg, kend)^T  for one workgroup.
//   * a wave owns one 16-row slab of W and walks K; lane l loads W[n0 + (l&15)][k + 8*(l>>4) .. +8], which IS the B fragment
//     of v_mfma_f32_16x16x32_bf16 (no LDS round trip for the read-once operand); 8 k-steps of loads are in flight per wave
//     before the first is consumed;
//   * the activations (the re-used operand) sit in LDS as [MT*16][256] K-tiles, swizzled (swz512_off); one fragment read
//     feeds MT MFMAs;
//   * fp32 accumulators stay in registers across the whole K range and are left to the caller's epilogue.
// What differs between the callers comes in a problem object P:
//   const bf16* a_row(int r)   where staged row r (0 <= r < MT*16) is read from; any readable row for r >= M
//   int M                      rows that count (rows past M are staged as zeros)
//   const void* w, const bf16* wscale    weight [N][K] (bf16, or fp8 codes) and its [N/128][K/128] block scales
//   int N, K, kbeg, kend       kend - kbeg need not be a multiple of the tile; K % 8 == 0
#pragma once

#include "gemm_plan.h"
#include "gemv_core.hip.h"
#include "mfma_common.hip.h"

namespace pgk {

static_assert(WS_KT == 256, "swz512_off: 512-byte rows");   // WS_KT (gemm_plan.h): K elements per LDS tile
constexpr int WS_THREADS = 256;   // 4 waves, 16 weight rows each

constexpr size_t ws_lds_bytes(int mt) { return (size_t)mt * 16 * WS_KT * 2; }

// n0: first weight row of this wave.  SKIP: row tiles wholly past M are not multiplied (the grouped kernel sizes MT for the
// fullest expert; the dense kernel has no such tiles and is built without the branch).  AHEAD: see the k-step loop.
template <int MT, bool FP8, bool SKIP, bool AHEAD, class P>
__device__ __forceinline__ void wsgemm_walk(const P& p, char* a_lds, int n0, f32x4_t (&acc)[MT]) {
    const int lane = threadIdx.x & 63;
    const int nrow = min(n0 + (lane & 15), p.N - 1);            // clamp: out-of-range rows are computed, never stored
    const int kl = 8 * (lane >> 4);
    const int mt_on = (p.M + 15) >> 4;

    // weight fragments of one K tile: 8 k-steps x 16 bytes per lane
    uint4 wreg[8];
    float wsc[8];
    auto load_w = [&](int kt) {
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int k = kt + s * 32 + kl;
            if constexpr (FP8) {
                // 8 codes per lane per k-step; dequantised to bf16 pairs when consumed
                const uint2 v = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint8_t*>(p.w) + (size_t)nrow * p.K + min(k, p.K - 8));
                wreg[s] = make_uint4(v.x, v.y, 0, 0);
                wsc[s] = to_f(p.wscale[(size_t)(nrow >> 7) * (p.K >> 7) + (min(k, p.K - 8) >> 7)]);
            } else {
                wreg[s] = load_nt16(reinterpret_cast<const bf16*>(p.w) + (size_t)nrow * p.K + min(k, p.K - 8));
            }
        }
    };
    // A tile staging: MT*16 x 32 chunks of 16 bytes, MT*2 per thread
    constexpr int ACH = MT * 16 * 32 / WS_THREADS;
    const bf16* arow[ACH];        // looked up once: the grouped kernel finds its rows through a table in memory
#pragma unroll
    for (int i = 0; i < ACH; ++i) arow[i] = p.a_row((threadIdx.x + i * WS_THREADS) >> 5);
    uint4 areg[ACH];
    auto load_a = [&](int kt) {
#pragma unroll
        for (int i = 0; i < ACH; ++i) {
            const int ch = threadIdx.x + i * WS_THREADS;
            const int k = kt + (ch & 31) * 8;
            // unconditional load from a clamped address, masked afterwards: a guarded load would be waited
            // for on the spot (16 serialised round trips per tile)
            // (the mask is applied in store_a: touching the value here would make the compiler wait for the next
            // tile's loads before this tile's MFMAs)
            areg[i] = *reinterpret_cast<const uint4*>(arow[i] + min(k, p.K - 8));
        }
    };
    auto store_a = [&](int kt) {
#pragma unroll
        for (int i = 0; i < ACH; ++i) {
            const int ch = threadIdx.x + i * WS_THREADS;
            const int r = ch >> 5, c = ch & 31;
            const bool ok = r < p.M && kt + c * 8 < p.kend;
            const uint4 v = areg[i];
            *reinterpret_cast<uint4*>(a_lds + swz512_off(r, c)) = make_uint4(ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u);
        }
    };

    load_w(p.kbeg);                      // HBM first: the longest latency in the kernel
    __builtin_amdgcn_sched_barrier(0);
    load_a(p.kbeg);
    for (int kt = p.kbeg; kt < p.kend; kt += WS_KT) {
        __syncthreads();          // previous tile fully consumed
        store_a(kt);
        __syncthreads();
        uint4 wcur[8];
        float scur[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) { wcur[s] = wreg[s]; scur[s] = wsc[s]; }
        if (kt + WS_KT < p.kend) { load_w(kt + WS_KT); load_a(kt + WS_KT); }   // next tile in flight during the MFMAs
        __builtin_amdgcn_sched_barrier(0);
        // AHEAD: A fragments are read one k-step ahead of the MFMAs that use them: with one wave per SIMD nothing else
        // hides the LDS latency (it costs MT*8 registers).  No K-tail branch: the A tile is zero beyond kend and the
        // clamped W loads are finite, so tail k-steps add exact zeros.
        uint4 af[2][AHEAD ? MT : 1];
        auto read_a1 = [&](int s, int mt) -> uint4 {
            return *reinterpret_cast<const uint4*>(a_lds + swz512_off(mt * 16 + (lane & 15), s * 4 + (lane >> 4)));
        };
        auto read_a = [&](int s) {
#pragma unroll
            for (int mt = 0; mt < (AHEAD ? MT : 0); ++mt) af[s & 1][mt] = read_a1(s, mt);
        };
        if constexpr (AHEAD) read_a(0);
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            if constexpr (AHEAD) {
                if (s + 1 < 8) read_a(s + 1);
                __builtin_amdgcn_sched_barrier(0);   // keep the MT reads ahead of this k-step's MFMAs
            }
            uint4 bfrag;
            if constexpr (FP8) bfrag = fp8x8_to_bf16x8(make_uint2(wcur[s].x, wcur[s].y), scur[s]);
            else bfrag = wcur[s];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                if (SKIP && mt >= mt_on) break;   // wave-uniform; without AHEAD a skipped tile is not read either
                uint4 a;
                if constexpr (AHEAD) a = af[s & 1][mt];
                else a = read_a1(s, mt);
                acc[mt] = mfma16<bf16>(a, bfrag, acc[mt]);
            }
            if constexpr (AHEAD) __builtin_amdgcn_sched_barrier(0);
        }
    }
}

}  // namespace pgk
