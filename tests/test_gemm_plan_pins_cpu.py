"""The host-side pickers of the GEMM family (csrc/gemm_plan.h) pinned through their query entry points, on a table of shapes
whose values were recorded before the pickers moved into that header: the weight-streaming row tile and the 192-column choice
through pgk_gemm_plan, the grouped GEMM's regime and K splits through pgk_grouped_gemm_sorted_splits, its tile-table size
through pgk_moe_max_tiles.  Needs no device.
Three moved pickers have no query entry point and so no pin here: wsgemm_pick_splits (the engine's prefill plan), moe_ws_pick_mt
(the grouped kernel's row-tile count; the MoE GPU tests reach all four values and compare outputs) and gemm256_swiglu_narrow
(the SwiGLU 96-column choice: both of its kernels compute the same values, so no test would notice a flipped choice)."""

from __future__ import annotations

import pytest

from pygpukit_amd import _hip
from pygpukit_amd.ops.matmul import gemm_plan, grouped_gemm_sorted_splits

# ((T, k, E, N, K), K splits, tile-table entries): both regimes, the 64-rows-per-expert regime edge (256 / 257 tokens at k = 2,
# E = 8; 1024 / 1025 at k = 8, E = 128), K below one LDS tile, K not a multiple of the tile, the 16-split cap
GROUPED_SPLITS = [
    ((1, 2, 8, 4096, 4096), 4, 9),
    ((3, 2, 8, 256, 384), 1, 9),
    ((12, 2, 8, 128, 384), 1, 9),
    ((25, 2, 8, 128, 640), 2, 9),
    ((40, 8, 16, 384, 512), 2, 19),
    ((64, 8, 128, 1536, 2048), 1, 132),
    ((64, 8, 128, 2048, 768), 1, 132),
    ((1, 8, 128, 2048, 768), 2, 129),
    ((8, 2, 8, 14336, 4096), 1, 9),
    ((8, 2, 8, 4096, 14336), 1, 9),
    ((256, 2, 8, 4096, 14336), 1, 12),
    ((257, 2, 8, 4096, 14336), 1, 13),
    ((1024, 8, 128, 2048, 768), 1, 192),
    ((1025, 8, 128, 2048, 768), 1, 193),
    ((2048, 2, 8, 256, 256), 1, 40),
    ((700, 4, 5, 384, 640), 1, 27),
    ((4, 1, 1, 64, 128), 1, 2),
    ((4, 1, 1, 64, 8192), 16, 2),
    ((16, 4, 60, 1408, 2048), 1, 61),
    ((5, 2, 8, 128, 200), 1, 9),
]

# ((op, M, N, K), leaf), bfloat16: every weight-streaming row tile at both of its edges, bf16 and fp8; the 192-column tiles
# where they fill the chip's rounds better and where they do not
DENSE_PLAN = [
    (("nt", 9, 320, 392), "wsgemm_mt1"),
    (("nt", 16, 320, 392), "wsgemm_mt1"),
    (("nt", 17, 1024, 1024), "wsgemm_mt2"),
    (("nt", 32, 1024, 1024), "wsgemm_mt2"),
    (("nt", 33, 320, 392), "wsgemm_mt4"),
    (("nt", 64, 1024, 1024), "wsgemm_mt4"),
    (("nt", 65, 320, 392), "wsgemm_mt8"),
    (("nt", 128, 1024, 1024), "wsgemm_mt8"),
    (("w8a16_nk", 5, 256, 384), "wsgemm_mt1_fp8"),
    (("w8a16_nk", 48, 256, 384), "wsgemm_mt4_fp8"),
    (("w8a16_nk", 128, 256, 384), "wsgemm_mt8_fp8"),
    (("nt", 2048, 6144, 1024), "gemm256s_n192"),
    (("nt", 2048, 3072, 1024), "gemm128s"),
    (("nt", 4096, 12288, 4096), "gemm256s"),
    (("nt", 8192, 9216, 1024), "gemm256s_n192"),
    (("nt", 8192, 1536, 1024), "gemm256s_n192"),
    (("nt", 12288, 4608, 512), "gemm256s_n192"),
    (("nt", 16384, 3072, 512), "gemm256s"),
    (("nt", 16384, 3264, 512), "gemm256s_n192"),
    (("w8a16_nk", 4096, 12288, 4096), "dequant+gemm256s"),
]


@pytest.mark.parametrize("shape, splits, tiles", GROUPED_SPLITS)
def test_grouped_pickers_keep_their_values(shape, splits, tiles):
    T, k, E, _, _ = shape
    assert grouped_gemm_sorted_splits(*shape) == splits
    assert int(_hip.load().pgk_moe_max_tiles(T, k, E)) == tiles


@pytest.mark.parametrize("call, leaf", DENSE_PLAN)
def test_dense_pickers_keep_their_values(call, leaf, monkeypatch):
    monkeypatch.delenv("PGK_GEMM256", raising=False)
    monkeypatch.delenv("PGK_GEMM256S", raising=False)
    assert gemm_plan(*call, "bfloat16") == leaf
