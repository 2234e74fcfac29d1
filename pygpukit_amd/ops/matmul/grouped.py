"""Grouped GEMM for Mixture-of-Experts (reference: src/pygpukit/ops/matmul/grouped.py:36-125 ->
grouped_gemm_fp8_bf16_sm120), on ops_moe.hip.

C[r, :] = A[r, :] @ W[e_r]^T with the experts' weights stacked [E, N, K].  Two ways to say which expert a row uses:
  * row_expert_ids [M] int32, rows in any order - the reference's contract (a plain kernel: not the hot path);
  * tiles= the table moe_compute_permutation returns (with expert_offsets=), rows already grouped by expert - the hot
    path MoELayer uses: each active expert's weight is streamed about once per call, experts without rows are not read.
The fp8 form dequantises to bf16 before the MFMA: at most 2^-9 relative per weight away from the reference's fp32
lut[code] * scale (the row-id form keeps the reference's fp32 arithmetic)."""

from __future__ import annotations

from pygpukit_amd import _hip
from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import bfloat16, float32, int32, uint8
from pygpukit_amd.ops._common import call


def grouped_gemm_init_lut() -> None:
    """The reference uploads an fp8 -> bf16 table; gfx950 converts e4m3 in hardware.  Nothing to do."""


def grouped_gemm_sorted_splits(num_tokens: int, k: int, num_experts: int, N: int, K: int) -> int:
    """K splits the sorted kernel uses for this shape: the leading dimension of its fp32 slab output (out_slabs=True)."""
    return int(_hip.load().pgk_grouped_gemm_sorted_splits(num_tokens, k, num_experts, N, K))


def _launch(a, b_stacked, b_scale, fp8, row_expert_ids, out, tiles, expert_offsets, permute_indices, top_k, out_slabs, name):
    M, K = a.shape
    E, N = b_stacked.shape[0], b_stacked.shape[1]
    if tiles is None:
        if out is None:
            out = GPUArray((M, N), bfloat16)
        call("pgk_grouped_gemm_rows", a._p, b_stacked._p, b_scale._p if fp8 else None, 1 if fp8 else 0, out._p,
             row_expert_ids._p, M, N, K, E, None)
        return out
    if expert_offsets is None or expert_offsets.dtype != int32 or expert_offsets.shape != (E + 1,):
        raise ValueError(f"{name}: tiles= needs expert_offsets int32 [{E + 1}]")
    if permute_indices is not None:        # A is the un-gathered x [T, K], read through the permutation
        T, k = M, top_k
        if permute_indices.dtype != int32 or permute_indices.shape != (T * k,):
            raise ValueError(f"{name}: permute_indices must be int32 [{T * k}]")
    else:
        T, k = M, 1
    rows = T * k
    from pygpukit_amd.ops.moe import moe_max_tiles
    if tiles.dtype != int32 or tiles.shape != (moe_max_tiles(T, k, E), 2):
        raise ValueError(f"{name}: tiles must be the int32 [{moe_max_tiles(T, k, E)}, 2] table of moe_compute_permutation")
    splits = grouped_gemm_sorted_splits(T, k, E, N, K) if out_slabs else 0
    shape, dt = ((splits, rows, N), float32) if out_slabs else ((rows, N), bfloat16)
    if out is None:
        out = GPUArray(shape, dt)
    elif out.shape != shape or out.dtype != dt:
        raise ValueError(f"out shape {out.shape} does not match expected {shape}")
    call("pgk_grouped_gemm_sorted", a._p, permute_indices._p if permute_indices is not None else None, b_stacked._p,
         b_scale._p if fp8 else None, 1 if fp8 else 0, out._p, splits, expert_offsets._p, tiles._p, T, k, E, N, K, None)
    return out


def grouped_gemm_fp8_bf16(
    a: GPUArray,
    b_stacked: GPUArray,
    b_scale: GPUArray,
    row_expert_ids: GPUArray | None,
    *,
    out: GPUArray | None = None,
    tiles: GPUArray | None = None,
    expert_offsets: GPUArray | None = None,
    permute_indices: GPUArray | None = None,
    top_k: int = 1,
    out_slabs: bool = False,
) -> GPUArray:
    """Grouped GEMM for MoE: C = A @ B_stacked^T with per-row expert IDs.

    Args:
        a: Input tokens [M, K], BF16.
        b_stacked: Stacked expert weights [num_experts, N, K], FP8 (uint8).
        b_scale: Block-wise scales [num_experts, N/128, K/128], BF16.
        row_expert_ids: Expert ID for each row [M], int32 (None with tiles=).
        out: Optional output tensor [M, N], BF16.
        tiles, expert_offsets: the sorted form (see the module docstring); permute_indices + top_k: A is x [T, K] and
            row r reads x[permute_indices[r] // top_k]; out_slabs: fp32 split-K slabs [S, rows, N] for moe_scatter.

    Returns:
        Output tensor [M, N], BF16.
    """
    if a.ndim != 2:
        raise ValueError(f"grouped_gemm_fp8_bf16 requires 2D input, got {a.ndim}D")
    if b_stacked.ndim != 3:
        raise ValueError(f"grouped_gemm_fp8_bf16 requires 3D weight, got {b_stacked.ndim}D")
    if a.dtype != bfloat16:
        raise ValueError(f"grouped_gemm_fp8_bf16 requires bfloat16 input, got {a.dtype}")
    if b_stacked.dtype != uint8:
        raise ValueError(f"grouped_gemm_fp8_bf16 requires uint8 (FP8) weights, got {b_stacked.dtype}")
    if b_scale.dtype != bfloat16:
        raise ValueError(f"grouped_gemm_fp8_bf16 requires bfloat16 scale, got {b_scale.dtype}")
    if tiles is None and (row_expert_ids is None or row_expert_ids.dtype != int32):
        raise ValueError(f"grouped_gemm_fp8_bf16 requires int32 row_expert_ids, got "
                         f"{None if row_expert_ids is None else row_expert_ids.dtype}")
    M = a.shape[0]
    K = a.shape[1]
    N = b_stacked.shape[1]
    if b_stacked.shape[2] != K:
        raise ValueError(f"grouped_gemm_fp8_bf16: K mismatch A[{M},{K}] vs B[...{N},{b_stacked.shape[2]}]")
    if tiles is None and row_expert_ids.shape[0] != M:
        raise ValueError(f"grouped_gemm_fp8_bf16: row_expert_ids size {row_expert_ids.shape[0]} != M ({M})")
    if out is not None and tiles is None:
        if out.shape != (M, N):
            raise ValueError(f"out shape {out.shape} does not match expected ({M}, {N})")
        if out.dtype != bfloat16:
            raise ValueError(f"out dtype {out.dtype} must be bfloat16")
    E = b_stacked.shape[0]
    if K % 128 or N % 128:
        raise ValueError(f"grouped_gemm_fp8_bf16: N={N} and K={K} must be multiples of the 128x128 scale block")
    if b_scale.shape != (E, N // 128, K // 128):
        raise ValueError(f"grouped_gemm_fp8_bf16: scale must be [{E}, {N // 128}, {K // 128}], got {b_scale.shape}")
    grouped_gemm_init_lut()
    return _launch(a, b_stacked, b_scale, True, row_expert_ids, out, tiles, expert_offsets, permute_indices, top_k, out_slabs,
                   "grouped_gemm_fp8_bf16")


grouped_gemm_fp8_bf16_sm120 = grouped_gemm_fp8_bf16


def grouped_gemm_bf16(
    a: GPUArray,
    b_stacked: GPUArray,
    row_expert_ids: GPUArray | None,
    *,
    out: GPUArray | None = None,
    tiles: GPUArray | None = None,
    expert_offsets: GPUArray | None = None,
    permute_indices: GPUArray | None = None,
    top_k: int = 1,
    out_slabs: bool = False,
) -> GPUArray:
    """bf16 experts: C = A @ B_stacked^T, B_stacked [num_experts, N, K] bf16, arguments as grouped_gemm_fp8_bf16.
    New here: the reference has no bf16 grouped path (its MoELayer runs bf16 experts one at a time behind a host sync)."""
    if a.ndim != 2:
        raise ValueError(f"grouped_gemm_bf16 requires 2D input, got {a.ndim}D")
    if b_stacked.ndim != 3:
        raise ValueError(f"grouped_gemm_bf16 requires 3D weight, got {b_stacked.ndim}D")
    if a.dtype != bfloat16 or b_stacked.dtype != bfloat16:
        raise ValueError(f"grouped_gemm_bf16 requires bfloat16 input and weights, got {a.dtype} and {b_stacked.dtype}")
    if tiles is None and (row_expert_ids is None or row_expert_ids.dtype != int32):
        raise ValueError("grouped_gemm_bf16 requires int32 row_expert_ids")
    M, K = a.shape
    N = b_stacked.shape[1]
    if b_stacked.shape[2] != K:
        raise ValueError(f"grouped_gemm_bf16: K mismatch A[{M},{K}] vs B[...{N},{b_stacked.shape[2]}]")
    if tiles is None and row_expert_ids.shape[0] != M:
        raise ValueError(f"grouped_gemm_bf16: row_expert_ids size {row_expert_ids.shape[0]} != M ({M})")
    if out is not None and tiles is None and (out.shape != (M, N) or out.dtype != bfloat16):
        raise ValueError(f"out must be bfloat16 ({M}, {N}), got {out.dtype} {out.shape}")
    if K % 8 or N % 8:
        raise ValueError(f"grouped_gemm_bf16: N={N} and K={K} must be multiples of 8")
    return _launch(a, b_stacked, None, False, row_expert_ids, out, tiles, expert_offsets, permute_indices, top_k, out_slabs,
                   "grouped_gemm_bf16")


__all__ = ["grouped_gemm_init_lut", "grouped_gemm_fp8_bf16", "grouped_gemm_fp8_bf16_sm120", "grouped_gemm_bf16",
           "grouped_gemm_sorted_splits"]
