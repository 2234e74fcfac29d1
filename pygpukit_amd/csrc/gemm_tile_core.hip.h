// The register-staged tile GEMM shared by gemm_mfma_kernel (ops_gemm.hip) and the grouped expert GEMM's many-rows regime
// (ops_moe.hip): BM x BN x 64 block tile, 256 threads = 2 x 2 waves, v_mfma_f32_16x16x32_{bf16,f16}, fp32 accumulate; A / B
// tiles staged global -> VGPR -> LDS (16-byte chunks, swz128_off), two LDS buffers: the global loads of tile t+1 are issued
// before the MFMAs of tile t and written to LDS after them (one barrier per K tile).  The TileRegs* types are the staging
// registers of one operand tile; gemm_tile_loop.hip.h is the loop; the caller says what to load and writes the accumulators out.
#pragma once

#include "gemv_core.hip.h"
#include "mfma_common.hip.h"

namespace pgk {

constexpr int GEMM_BK = 64;       // K elements per tile (128 bytes per LDS row)
constexpr int GEMM_THREADS = 256;

// ---- A-side (and NT B-side) tile: rows x 64 elements, k contiguous in memory -----------------
template <int ROWS>
struct TileRegsK {
    static constexpr int CH = ROWS * 8 / GEMM_THREADS;  // 16-byte chunks per thread
    uint4 v[CH > 0 ? CH : 1];
    template <class T>
    __device__ __forceinline__ void load(const T* base, int row0, int nrows, int k0, int K, int ld) {
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int c = threadIdx.x + i * GEMM_THREADS;
            const int r = c >> 3, kc = c & 7;
            const int gr = row0 + r, gk = k0 + kc * 8;
            if (gr < nrows && gk < K) v[i] = *reinterpret_cast<const uint4*>(base + (size_t)gr * ld + gk);
            else v[i] = make_uint4(0, 0, 0, 0);
        }
    }
    // gathered rows: rows[i] is where this thread's chunk i (tile row (threadIdx.x + i * 256) >> 3) starts, always readable; a row
    // that does not count is zeroed by store_rows, so that the loads depend on k alone and issue together
    template <class T>
    __device__ __forceinline__ void load_rows(const T* const (&rows)[CH > 0 ? CH : 1], int k0, int K) {
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int gk = k0 + ((threadIdx.x + i * GEMM_THREADS) & 7) * 8;
            v[i] = gk < K ? *reinterpret_cast<const uint4*>(rows[i] + gk) : make_uint4(0, 0, 0, 0);
        }
    }
    __device__ __forceinline__ void store_rows(char* lds, const bool (&keep)[CH > 0 ? CH : 1]) const {
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int c = threadIdx.x + i * GEMM_THREADS;
            *reinterpret_cast<uint4*>(lds + swz128_off(c >> 3, c & 7)) = keep[i] ? v[i] : make_uint4(0, 0, 0, 0);
        }
    }
    __device__ __forceinline__ void store(char* lds) const {
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int c = threadIdx.x + i * GEMM_THREADS;
            *reinterpret_cast<uint4*>(lds + swz128_off(c >> 3, c & 7)) = v[i];
        }
    }
};

// ---- NN B-side tile: B[K,N] row-major; tile is 64 k-rows x BN columns, transposed into LDS ----
template <int BN>
struct TileRegsN {
    static constexpr int CH = 64 * (BN / 8) / GEMM_THREADS;
    uint4 v[CH];
    template <class T>
    __device__ __forceinline__ void load(const T* base, int n0, int N, int k0, int K) {
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int c = threadIdx.x + i * GEMM_THREADS;
            const int k = c / (BN / 8), nc = c % (BN / 8);
            const int gk = k0 + k, gn = n0 + nc * 8;
            if (gk < K && gn < N) v[i] = *reinterpret_cast<const uint4*>(base + (size_t)gk * N + gn);  // N % 8 == 0
            else v[i] = make_uint4(0, 0, 0, 0);
        }
    }
    __device__ __forceinline__ void store(char* lds) const {
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int c = threadIdx.x + i * GEMM_THREADS;
            const int k = c / (BN / 8), nc = c % (BN / 8);
            const uint32_t w[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int n = nc * 8 + j;
                const uint16_t e = (uint16_t)((j & 1) ? (w[j >> 1] >> 16) : (w[j >> 1] & 0xFFFFu));
                *reinterpret_cast<uint16_t*>(lds + swz128_off(n, k >> 3) + (k & 7) * 2) = e;
            }
        }
    }
};

// ---- fp8 B tiles, dequantised to bf16 on the way into LDS -----------------------------------
// NT: W[N,K] u8, scale[N/128, K/128] bf16.  One 16-byte load = 16 k-values of one row.
template <int BN>
struct TileRegsFp8NT {
    static constexpr int CH = (BN * 4 + GEMM_THREADS - 1) / GEMM_THREADS;  // 4 x 16-code chunks per row
    uint4 v[CH];
    float sc[CH];
    __device__ __forceinline__ void load(const uint8_t* w, const bf16* scale, int n0, int N, int k0, int K) {
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int c = threadIdx.x + i * GEMM_THREADS;
            const int r = c >> 2, q = c & 3;
            const int gn = n0 + r, gk = k0 + q * 16;
            if (c < BN * 4 && gn < N && gk < K) {
                v[i] = *reinterpret_cast<const uint4*>(w + (size_t)gn * K + gk);
                sc[i] = to_f(scale[(size_t)(gn >> 7) * (K >> 7) + (gk >> 7)]);
            } else {
                v[i] = make_uint4(0, 0, 0, 0);
                sc[i] = 0.f;
            }
        }
    }
    __device__ __forceinline__ void store(char* lds) const {
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int c = threadIdx.x + i * GEMM_THREADS;
            if (c >= BN * 4) continue;
            const int r = c >> 2, q = c & 3;
            *reinterpret_cast<uint4*>(lds + swz128_off(r, q * 2)) = fp8x8_to_bf16x8(make_uint2(v[i].x, v[i].y), sc[i]);
            *reinterpret_cast<uint4*>(lds + swz128_off(r, q * 2 + 1)) = fp8x8_to_bf16x8(make_uint2(v[i].z, v[i].w), sc[i]);
        }
    }
};
// KN: B[K,N] u8, scale[K/128, N/128].  One 16-byte load = 16 n-values of one k.
template <int BN>
struct TileRegsFp8KN {
    static constexpr int PER_ROW = BN / 16;
    static constexpr int CH = (64 * PER_ROW + GEMM_THREADS - 1) / GEMM_THREADS;
    uint4 v[CH];
    float sc[CH];
    __device__ __forceinline__ void load(const uint8_t* b, const bf16* scale, int n0, int N, int k0, int K) {
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int c = threadIdx.x + i * GEMM_THREADS;
            const int k = c / PER_ROW, nc = c % PER_ROW;
            const int gk = k0 + k, gn = n0 + nc * 16;
            if (c < 64 * PER_ROW && gk < K && gn < N) {
                v[i] = *reinterpret_cast<const uint4*>(b + (size_t)gk * N + gn);  // N % 16 == 0
                sc[i] = to_f(scale[(size_t)(gk >> 7) * (N >> 7) + (gn >> 7)]);
            } else {
                v[i] = make_uint4(0, 0, 0, 0);
                sc[i] = 0.f;
            }
        }
    }
    // (element by element: the 16 values of a chunk go to 16 different LDS rows, so there is no fragment to pack)
    __device__ __forceinline__ void store(char* lds) const {
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int c = threadIdx.x + i * GEMM_THREADS;
            if (c >= 64 * PER_ROW) continue;
            const int k = c / PER_ROW, nc = c % PER_ROW;
            float f[16];
            WTraits<fp8e4m3>::decode(v[i], f);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int n = nc * 16 + j;
                *reinterpret_cast<uint16_t*>(lds + swz128_off(n, k >> 3) + (k & 7) * 2) = f_to_bf16_bits(f[j] * sc[i]);
            }
        }
    }
};

// LDS: [2][BM rows] A then [2][BN rows] B, 128 bytes per row
constexpr size_t gemm_tile_lds_bytes(int bm, int bn) { return 2 * (size_t)(bm + bn) * 128; }
template <int BM, int BN> __device__ __forceinline__ char* gemm_tile_a(char* smem, int buf) { return smem + buf * (BM * 128); }
template <int BM, int BN> __device__ __forceinline__ char* gemm_tile_b(char* smem, int buf) { return smem + 2 * (BM * 128) + buf * (BN * 128); }

// The loop itself is gemm_tile_loop.hip.h, text that a kernel includes in its body: as a function over these types hipcc
// schedules the small-tile dense kernels' prologues differently (+1 .. 4 per cent instructions on 23 of 78 instantiations),
// as text in the kernel it does not.

}  // namespace pgk
