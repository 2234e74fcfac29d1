// The double-buffered main loop of the register-staged tile GEMM (gemm_tile_core.hip.h), as text: a kernel includes this
// file once, inside its body, after it has declared
//   T                         element type of the MFMA (bf16 or f16);  constexpr int BM, BN, the block tile
//   char* / char[] smem       gemm_tile_lds_bytes(BM, BN) bytes of LDS
//   int lane, wm, wn          threadIdx.x & 63, wave >> 1, wave & 1
//   int kbeg, kend            the K range
//   load_tiles(int k0)        fills the kernel's staging registers with the A and B tiles at k0
//   store_tiles(int buf)      writes them to gemm_tile_a / gemm_tile_b<BM, BN>(smem, buf) (the buffer index and not the two
//                             addresses: handed the addresses, hipcc keeps them in registers instead of folding them into
//                             the stores' offsets)
//   f32x4_t acc[BM / 32][BN / 32]   the wave's accumulators, zeroed
// and reads acc afterwards: acc[i][j] is the 16 x 16 tile at (wm * BM/2 + i * 16, wn * BN/2 + j * 16), C/D map of
// v_mfma_f32_16x16x32 (col = lane & 15, row = (lane >> 4) * 4 + reg).
// It is not a function because hipcc does not compile it the same way as one (see gemm_tile_core.hip.h).  No include guard.
{
    constexpr int GT_WM = BM / 2, GT_WN = BN / 2, GT_TM = GT_WM / 16, GT_TN = GT_WN / 16;
    const int nk = (kend - kbeg + GEMM_BK - 1) / GEMM_BK;
    load_tiles(kbeg);
    store_tiles(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) load_tiles(kbeg + (kt + 1) * GEMM_BK);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            uint4 fa[GT_TM], fb[GT_TN];
            const int kc = ks * 4 + (lane >> 4);
#pragma unroll
            for (int i = 0; i < GT_TM; ++i)
                fa[i] = *reinterpret_cast<const uint4*>(gemm_tile_a<BM, BN>(smem, buf) + swz128_off(wm * GT_WM + i * 16 + (lane & 15), kc));
#pragma unroll
            for (int j = 0; j < GT_TN; ++j)
                fb[j] = *reinterpret_cast<const uint4*>(gemm_tile_b<BM, BN>(smem, buf) + swz128_off(wn * GT_WN + j * 16 + (lane & 15), kc));
#pragma unroll
            for (int i = 0; i < GT_TM; ++i)
#pragma unroll
                for (int j = 0; j < GT_TN; ++j) acc[i][j] = mfma16<T>(fa[i], fb[j], acc[i][j]);
        }
        if (kt + 1 < nk) store_tiles(buf ^ 1);
        __syncthreads();
    }
}
