// LDS-DMA (global_load_lds_*): a wave-instruction moves 64 lanes x {16, 4, 2} bytes from global memory straight into LDS - no
// staging registers, no ds_write pass.  Lane l's bytes land at lds_addr + l x max(size, 4): a sub-dword transfer still strides
// the lanes by 4 bytes (zero-extended), and lds_addr is wave-uniform (it travels in m0).
//
// Written as inline asm on purpose: issued through __builtin_amdgcn_global_load_lds, hipcc (ROCm 7.2) puts an
// s_waitcnt vmcnt(0) in front of the next ds_read of the kernel - it cannot tell the buffer being filled from the
// buffer being read - and the prefetch is drained the moment it is issued.  The compiler does not count these loads either:
// the waits that order a DMA before the reads of its bytes are the explicit vmcnt (+ barrier) pairs of the kernel that issued it.
#pragma once
#include <cstdint>

namespace pgk {

// the 32-bit LDS address of a __shared__ object, as m0 wants it
__device__ __forceinline__ uint32_t lds_addr_of(const void* p) {
    return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const char*)p;
}

// Two forms per size: per-lane 64-bit global addresses, or (_so) a wave-uniform 64-bit base in an SGPR pair plus a per-lane
// 32-bit byte offset - half the address registers and no 64-bit arithmetic per lane.
#define PGK_LDS_DMA(NAME, OP)                                                                                                        \
    __device__ __forceinline__ void NAME(const void* src, uint32_t lds_addr) {                                                       \
        asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\t" OP " %0, off" ::"v"(src), "s"(lds_addr) : "memory", "m0");                     \
    }                                                                                                                                \
    __device__ __forceinline__ void NAME##_so(const void* sbase, uint32_t voff, uint32_t lds_addr) {                                 \
        asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\t" OP " %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_addr) : "memory", "m0");         \
    }
PGK_LDS_DMA(lds_dma16, "global_load_lds_dwordx4")
PGK_LDS_DMA(lds_dma4, "global_load_lds_dword")
PGK_LDS_DMA(lds_dma2, "global_load_lds_ushort")
#undef PGK_LDS_DMA

}  // namespace pgk
