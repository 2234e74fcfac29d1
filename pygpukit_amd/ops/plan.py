"""[build-defined] Host-side queries of the base op dispatch (csrc/base_plan.h): which kernel branch an elementwise op, a
row norm, RoPE, clamp or where takes, and how many blocks it launches.  Both are computed by the functions the launchers
themselves call and need no device.  The leaves are listed in DESIGN.md ("Base op dispatch leaves").  The same pair of queries
for the byte movers (csrc/tensor_plan.h; DESIGN.md "Byte-mover dispatch leaves"): tensor_op_plan / tensor_op_grid."""

from __future__ import annotations

BASE_PLAN_OPS = ("binary", "activation", "glu", "glu_packed", "bias_add", "cast", "rmsnorm", "rmsnorm_residual", "layernorm",
                 "rope", "clamp", "where", "reduce")


def _query(fn: str, op: str, n_or_rows: int, features: int, dtype, aligned: bool):
    from pygpukit_amd import _hip
    from pygpukit_amd.core.dtypes import as_dtype

    lib = _hip.load()
    got = getattr(lib, fn)(str(op).encode(), max(int(n_or_rows), 0), int(features), as_dtype(dtype).code, int(bool(aligned)))
    if got is None or (isinstance(got, int) and got < 0):
        msg = lib.pgk_last_error()
        raise ValueError(msg.decode(errors="replace") if msg else f"{fn}: invalid call op={op} n={n_or_rows} features={features} dtype={dtype}")
    return got


def base_op_plan(op: str, rows: int, features: int, dtype, aligned: bool = True) -> str:
    """The kernel branch of a base op: ew_vec / ew_scalar (binary, activation, glu), row_vec / row_scalar (glu_packed with
    features = inter, bias_add), norm_wave / norm_block (rmsnorm, rmsnorm_residual, layernorm), cast_x4, rope_pairs (rows =
    seq * (Hq + Hk), features = D), ew_stride (clamp, where), reduce_tree (sum, mean, max, min: the first level).  `rows` is
    the element count for the flat ops, which ignore `features`.  `aligned=False`: one of the pointers the launcher tests is
    off 16-byte alignment."""
    return _query("pgk_base_op_plan", op, rows, features, dtype, aligned).decode()


def base_op_grid(op: str, n_or_rows: int, features: int, dtype, aligned: bool = True) -> int:
    """The number of blocks the launcher of `op` starts for this call (256 threads each); arguments as base_op_plan."""
    return int(_query("pgk_base_op_grid", op, n_or_rows, features, dtype, aligned))


# ---- the byte movers (csrc/tensor_plan.h) --------------------------------------------------------------------------------------
TENSOR_PLAN_OPS = ("transpose_2d", "transpose_batched", "transpose_3d_021", "repeat_interleave", "split_qkv", "embedding_lookup",
                   "slice_rows", "kv_cache_write", "argmax", "paged_cache_write", "scatter_last_logits")


def _low_bits(ptrs) -> int:
    bits = 0
    for p in ptrs:
        bits |= int(p.data_ptr() if hasattr(p, "data_ptr") else p)
    return bits & 15


def _tensor_query(fn: str, op: str, rows: int, row_bytes: int, itemsize: int, ptrs, batch: int, widths):
    from pygpukit_amd import _hip

    lib = _hip.load()
    bits = _low_bits(ptrs)
    if widths is not None:
        if str(op) != "split_qkv" or len(widths) != 3 or sum(int(w) for w in widths) != int(row_bytes):
            raise ValueError(f"{fn}: widths are the q, k and v byte sizes of a split_qkv row of {row_bytes} bytes, got {widths} for {op}")
        bits |= (int(widths[0]) | int(widths[1]) | int(widths[2])) & 15
    elif str(op) == "split_qkv":
        raise ValueError(f"{fn}: split_qkv needs widths=(q_bytes, k_bytes, v_bytes)")
    got = getattr(lib, fn)(str(op).encode(), max(int(batch), 0), max(int(rows), 0), max(int(row_bytes), 0), int(itemsize), bits)
    if got is None or (isinstance(got, int) and got < 0):
        msg = lib.pgk_last_error()
        raise ValueError(msg.decode(errors="replace") if msg else f"{fn}: invalid call op={op} rows={rows} row_bytes={row_bytes}")
    return got


def tensor_op_plan(op: str, rows: int, row_bytes: int, itemsize: int = 1, ptrs=(), *, batch: int = 1, widths=None) -> str:
    """The kernel instantiation of a byte mover: vec16 / vec8 / vec4 / vec2 / vec1 (transpose_3d_021, which transpose_4d_0213
    launches once per slab, repeat_interleave, slice_rows, kv_cache_write, embedding_lookup, scatter_last_logits, split_qkv,
    paged_cache_write: always vec16), tile64 (transpose_2d, transpose_batched with `batch` matrices), block256 / block1024
    (argmax).  `rows` counts the output rows of `row_bytes` bytes (kv_cache_write: seq * cache heads; paged_cache_write:
    tokens * kv heads; the transposes: the matrix is rows x row_bytes / itemsize).  `ptrs`: the arrays or addresses the launcher
    tests - input and output; qkv, q, k, v - of which the low four bits count.  split_qkv also takes widths=(q_bytes, k_bytes,
    v_bytes), which sum to row_bytes."""
    return _tensor_query("pgk_tensor_op_plan", op, rows, row_bytes, itemsize, ptrs, batch, widths).decode()


def tensor_op_grid(op: str, rows: int, row_bytes: int, itemsize: int = 1, ptrs=(), *, batch: int = 1, widths=None) -> int:
    """The number of blocks the launcher of `op` starts for this call (256 threads each; argmax: as the leaf says); arguments as
    tensor_op_plan.  The grid-stride movers cap it at 4096."""
    return int(_tensor_query("pgk_tensor_op_grid", op, rows, row_bytes, itemsize, ptrs, batch, widths))


__all__ = ["base_op_plan", "base_op_grid", "BASE_PLAN_OPS", "tensor_op_plan", "tensor_op_grid", "TENSOR_PLAN_OPS"]
