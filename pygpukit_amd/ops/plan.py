"""[build-defined] Host-side queries of the base op dispatch (csrc/base_plan.h): which kernel branch an elementwise op, a
row norm, RoPE, clamp or where takes, and how many blocks it launches.  Both are computed by the functions the launchers
themselves call and need no device.  The leaves are listed in DESIGN.md ("Base op dispatch leaves")."""

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


__all__ = ["base_op_plan", "base_op_grid", "BASE_PLAN_OPS"]
