// The vocabulary every MFMA GEMM kernel of this library shares: operand vector types, the 16 x 16 x 32 MFMA per element
// type, the two XOR swizzles of the LDS tiles and the fp8 fragment dequantisation.  (The flash / attention headers keep
// their own typedefs.)
#pragma once

#include "pgk_device.hip.h"

namespace pgk {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef int i32x8_t __attribute__((ext_vector_type(8)));

template <class T> __device__ __forceinline__ f32x4_t mfma16(const uint4& a, const uint4& b, f32x4_t c);
template <> __device__ __forceinline__ f32x4_t mfma16<bf16>(const uint4& a, const uint4& b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}
template <> __device__ __forceinline__ f32x4_t mfma16<f16>(const uint4& a, const uint4& b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
}

// Byte offset of 16-byte chunk `kc` (0..7) of row `row` in a tile of 128-byte rows (64 x 16-bit, or 128 x 8-bit).  A
// fragment read takes the same chunk of 16 consecutive rows: unswizzled those sit 128 bytes apart and fall on the same two
// 16-byte slots of the banks; XOR-ing the chunk with the row's low 3 bits gives 8 consecutive rows 8 different chunks, so
// the ds_read_b128 fragment reads (and the staging ds_write_b128) are bank-conflict free.
__device__ __forceinline__ int swz128_off(int row, int kc) { return row * 128 + ((kc ^ (row & 7)) << 4); }

// Byte offset of 16-byte chunk `c` (0..31) of row `r` in the weight-streaming A tile of 512-byte rows (256 x bf16).  Rows
// are a whole number of bank sweeps apart, so the 16 rows of an A fragment would all hit the same banks; XOR-ing the low 4
// chunk bits with the row puts them on 16 different 16-byte slots.  Bit 4 of the chunk (which half of the row) stays.
__device__ __forceinline__ int swz512_off(int r, int c) { return r * 512 + (((c & ~15) | ((c ^ r) & 15)) << 4); }

// 8 fp8-e4m3 codes (OCP, v_cvt_pk_f32_fp8) times one block scale -> 8 bf16 in the same order: the multiply in fp32, then
// one rounding per element (v_cvt_pk_bf16_f32).  This is the B fragment of a w8a16 MFMA.
__device__ __forceinline__ uint4 fp8x8_to_bf16x8(uint2 codes, float scale) {
    const pgk_f32x2 a0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)codes.x, false), a1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)codes.x, true);
    const pgk_f32x2 a2 = __builtin_amdgcn_cvt_pk_f32_fp8((int)codes.y, false), a3 = __builtin_amdgcn_cvt_pk_f32_fp8((int)codes.y, true);
    return make_uint4(pack_bf16x2(a0.x * scale, a0.y * scale), pack_bf16x2(a1.x * scale, a1.y * scale),
                      pack_bf16x2(a2.x * scale, a2.y * scale), pack_bf16x2(a3.x * scale, a3.y * scale));
}

}  // namespace pgk
