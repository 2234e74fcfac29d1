"""Mixture-of-Experts routing ops (reference: native/bindings/moe.cpp -> native/ops/moe/*.cuh), on ops_moe.hip.

The reference's native names and argument orders are kept: moe_topk_with_indices, moe_softmax_topk,
moe_compute_permutation, moe_gather, moe_scatter, moe_expand_expert_offsets.  moe_topk_softmax is the fused form of the
first two, which MoELayer uses.  One difference is deliberate: moe_compute_permutation is a stable counting sort, so
within one expert the sorted rows are in ascending flat index (token * k + slot) and two runs give identical results;
the reference's order within an expert is whatever its atomicAdd produced."""

from __future__ import annotations

from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import bfloat16, float16, float32, int32
from pygpukit_amd.ops._common import call

MAX_EXPERTS = 256
MAX_TOPK = 8


def _check_i32(a: GPUArray, shape, name: str, what: str) -> None:
    if a.dtype != int32:
        raise ValueError(f"{name}: {what} must be int32, got {a.dtype}")
    if a.shape != tuple(shape):
        raise ValueError(f"{name}: {what} shape {a.shape} does not match expected {tuple(shape)}")


def _check_routing_logits(logits: GPUArray, values: GPUArray, indices: GPUArray, k: int, name: str) -> tuple[int, int]:
    if logits.ndim != 2:
        raise ValueError(f"{name}: logits must be 2D [num_tokens, num_experts]")
    if logits.dtype not in (bfloat16, float32):
        raise ValueError(f"{name}: logits must be bfloat16 or float32, got {logits.dtype}")
    T, E = logits.shape
    if not 1 <= E <= MAX_EXPERTS:
        raise ValueError(f"{name}: num_experts={E} outside [1, {MAX_EXPERTS}]")
    if not 1 <= k <= min(MAX_TOPK, E):
        raise ValueError(f"{name}: k={k} outside [1, min({MAX_TOPK}, num_experts={E})]")
    if values.shape != (T, k) or values.dtype != logits.dtype:
        raise ValueError(f"{name}: values must be {logits.dtype} [{T}, {k}], got {values.dtype} {values.shape}")
    _check_i32(indices, (T, k), name, "indices")
    return T, E


def moe_topk_with_indices(logits: GPUArray, values: GPUArray, indices: GPUArray, k: int) -> None:
    """values/indices [T, k] = the k largest logits of each row, descending; the lowest expert index first among equal
    logits (topk_with_indices_kernel)."""
    T, E = _check_routing_logits(logits, values, indices, k, "moe_topk_with_indices")
    call("pgk_moe_topk_softmax", logits._p, values._p, indices._p, T, E, k, 0, logits.dtype.code, None)


def moe_softmax_topk(values: GPUArray, k: int) -> None:
    """In place: each row of values [T, k] becomes its softmax (fp32 math, stored in the values dtype)."""
    if values.ndim != 2 or values.shape[1] != k:
        raise ValueError("moe_softmax_topk: values must be 2D [num_tokens, k]")
    if values.dtype not in (bfloat16, float32):
        raise ValueError(f"moe_softmax_topk: values must be bfloat16 or float32, got {values.dtype}")
    if not 1 <= k <= MAX_TOPK:
        raise ValueError(f"moe_softmax_topk: k={k} outside [1, {MAX_TOPK}]")
    call("pgk_moe_softmax_topk", values._p, values.shape[0], k, values.dtype.code, None)


def moe_topk_softmax(logits: GPUArray, weights: GPUArray, indices: GPUArray, k: int) -> None:
    """moe_topk_with_indices followed by moe_softmax_topk, in one launch."""
    T, E = _check_routing_logits(logits, weights, indices, k, "moe_topk_softmax")
    call("pgk_moe_topk_softmax", logits._p, weights._p, indices._p, T, E, k, 1, logits.dtype.code, None)


def moe_max_tiles(num_tokens: int, k: int, num_experts: int) -> int:
    """Rows of the tile table moe_compute_permutation writes: ceil(T*k / 128) + E."""
    from pygpukit_amd import _hip
    return int(_hip.load().pgk_moe_max_tiles(num_tokens, k, num_experts))


def moe_compute_permutation(expert_indices: GPUArray, expert_counts: GPUArray, expert_offsets: GPUArray,
                            permute_indices: GPUArray, reverse_perm: GPUArray, num_experts: int, k: int, *,
                            tiles: GPUArray | None = None) -> GPUArray:
    """Sort the T*k (token, slot) entries by expert, stably.  Writes expert_counts [E], expert_offsets [E+1],
    permute_indices [T*k] (sorted row -> token * k + slot), reverse_perm [T*k] (the inverse), and the tile table
    [moe_max_tiles(T, k, E), 2] that grouped_gemm_bf16 / grouped_gemm_fp8_bf16 take as `tiles`; returns the table."""
    from pygpukit_amd import _hip
    name = "moe_compute_permutation"
    if expert_indices.dtype != int32:
        raise ValueError(f"{name}: expert_indices must be int32")
    if expert_indices.ndim != 2 or expert_indices.shape[1] != k:
        raise ValueError(f"{name}: expert_indices must be 2D [num_tokens, k={k}], got {expert_indices.shape}")
    if not 1 <= num_experts <= MAX_EXPERTS:
        raise ValueError(f"{name}: num_experts={num_experts} outside [1, {MAX_EXPERTS}]")
    T = expert_indices.shape[0]
    _check_i32(expert_counts, (num_experts,), name, "expert_counts")
    _check_i32(expert_offsets, (num_experts + 1,), name, "expert_offsets")
    _check_i32(permute_indices, (T * k,), name, "permute_indices")
    _check_i32(reverse_perm, (T * k,), name, "reverse_perm")
    n_tiles = moe_max_tiles(T, k, num_experts)
    if tiles is None:
        tiles = GPUArray((n_tiles, 2), int32)
    _check_i32(tiles, (n_tiles, 2), name, "tiles")
    ws_bytes = int(_hip.load().pgk_moe_workspace_bytes(T, k, num_experts))
    ws = GPUArray((max(ws_bytes // 4, 1),), int32)
    call("pgk_moe_compute_permutation", expert_indices._p, T, k, num_experts, expert_counts._p, expert_offsets._p,
         permute_indices._p, reverse_perm._p, tiles._p, ws._p, None)
    return tiles


def moe_gather(hidden: GPUArray, permute_indices: GPUArray, gathered: GPUArray, k: int) -> None:
    """gathered [T*k, H] = hidden[permute_indices[r] // k] (the sorted order)."""
    if hidden.ndim != 2:
        raise ValueError("moe_gather: hidden must be 2D")
    if hidden.dtype not in (bfloat16, float16, float32):
        raise ValueError(f"moe_gather: unsupported dtype {hidden.dtype}")
    T, H = hidden.shape
    _check_i32(permute_indices, (T * k,), "moe_gather", "permute_indices")
    if gathered.shape != (T * k, H) or gathered.dtype != hidden.dtype:
        raise ValueError(f"moe_gather: gathered must be {hidden.dtype} [{T * k}, {H}], got {gathered.dtype} {gathered.shape}")
    call("pgk_moe_gather", hidden._p, permute_indices._p, gathered._p, T, k, H, hidden.dtype.code, None)


def moe_scatter(expert_outputs: GPUArray, router_weights: GPUArray, reverse_perm: GPUArray, output: GPUArray, k: int) -> None:
    """output [T, H] = sum over slot of router_weights[t, slot] * expert_outputs[reverse_perm[t*k + slot]], summed in
    fp32 in slot order and rounded once.  expert_outputs may also be fp32 split-K slabs [S, T*k, H] (summed first)."""
    if output.ndim != 2:
        raise ValueError("moe_scatter: output must be 2D")
    if output.dtype not in (bfloat16, float16, float32):
        raise ValueError(f"moe_scatter: unsupported dtype {output.dtype}")
    T, H = output.shape
    if router_weights.shape != (T, k) or router_weights.dtype != output.dtype:
        raise ValueError(f"moe_scatter: router_weights must be {output.dtype} [{T}, {k}], got {router_weights.dtype} "
                         f"{router_weights.shape}")
    _check_i32(reverse_perm, (T * k,), "moe_scatter", "reverse_perm")
    if expert_outputs.ndim == 3 and expert_outputs.dtype == float32 and expert_outputs.shape[1:] == (T * k, H):
        splits = expert_outputs.shape[0]
    elif expert_outputs.shape == (T * k, H) and expert_outputs.dtype == output.dtype:
        splits = 0
    else:
        raise ValueError(f"moe_scatter: expert_outputs must be {output.dtype} [{T * k}, {H}] or float32 [S, {T * k}, {H}], "
                         f"got {expert_outputs.dtype} {expert_outputs.shape}")
    call("pgk_moe_scatter", expert_outputs._p, splits, router_weights._p, reverse_perm._p, output._p, T, k, H,
         output.dtype.code, None)


def moe_expand_expert_offsets(expert_offsets: GPUArray, row_expert_ids: GPUArray, num_experts: int) -> None:
    """row_expert_ids [M] = the expert whose segment [offsets[e], offsets[e+1]) holds row r (-1 past offsets[E])."""
    if expert_offsets.dtype != int32:
        raise ValueError("moe_expand_expert_offsets: expert_offsets must be int32")
    if row_expert_ids.dtype != int32:
        raise ValueError("moe_expand_expert_offsets: row_expert_ids must be int32")
    if expert_offsets.shape != (num_experts + 1,):
        raise ValueError("moe_expand_expert_offsets: expert_offsets size mismatch")
    if row_expert_ids.ndim != 1:
        raise ValueError("moe_expand_expert_offsets: row_expert_ids must be 1D")
    call("pgk_moe_expand_expert_offsets", expert_offsets._p, num_experts, row_expert_ids._p, row_expert_ids.shape[0], None)


__all__ = ["moe_topk_with_indices", "moe_softmax_topk", "moe_topk_softmax", "moe_compute_permutation", "moe_gather",
           "moe_scatter", "moe_expand_expert_offsets", "moe_max_tiles"]
