"""Linear-layer helpers (reference: src/pygpukit/ops/nn/linear.py:14-159 -> ops.cuh:139,271,410)."""

from __future__ import annotations

import ctypes as C

from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import int32
from pygpukit_amd.ops._common import call, validate_float, validate_same_dtype


def bias_add_inplace(output: GPUArray, bias: GPUArray) -> None:
    """output[batch, features] += bias[features]."""
    validate_float(output, "bias_add_inplace")
    if output.ndim != 2 or bias.ndim != 1 or bias.shape[0] != output.shape[1]:
        raise ValueError(f"bias_add_inplace: output {output.shape} / bias {bias.shape} mismatch")
    validate_same_dtype(output, bias, "bias_add_inplace")
    call("pgk_bias_add_inplace", output._p, bias._p, output.shape[0], output.shape[1], output.dtype.code, None)


def split_qkv_batch(qkv: GPUArray, q_out: GPUArray, k_out: GPUArray, v_out: GPUArray, q_dim: int, k_dim: int, v_dim: int) -> None:
    """qkv [rows, q+k+v] -> q_out [rows, q_dim...], k_out, v_out (pre-allocated, any trailing shape)."""
    if qkv.ndim != 2 or qkv.shape[1] != q_dim + k_dim + v_dim:
        raise ValueError(f"split_qkv_batch: qkv {qkv.shape} != [rows, {q_dim + k_dim + v_dim}]")
    rows = qkv.shape[0]
    for o, d, n in ((q_out, q_dim, "q_out"), (k_out, k_dim, "k_out"), (v_out, v_dim, "v_out")):
        if o.size != rows * d or o.dtype != qkv.dtype:
            raise ValueError(f"split_qkv_batch: {n} {o.shape}/{o.dtype} does not hold [{rows}, {d}] of {qkv.dtype}")
    call("pgk_split_qkv_batch", qkv._p, q_out._p, k_out._p, v_out._p, rows, q_dim, k_dim, v_dim, qkv.itemsize, None)


def slice_rows_range_ptr(table: GPUArray, out: GPUArray, start_pos_buf: GPUArray, count: int) -> None:
    """out[0:count, :] = table[start:start+count, :], start read from a device int32."""
    if table.ndim != 2 or out.ndim != 2 or out.shape[1] != table.shape[1] or out.shape[0] < count:
        raise ValueError(f"slice_rows_range_ptr: table {table.shape} / out {out.shape} / count {count} mismatch")
    validate_same_dtype(table, out, "slice_rows_range_ptr")
    if start_pos_buf.dtype != int32:
        raise ValueError("slice_rows_range_ptr: start_pos_buf must be int32")
    call("pgk_slice_rows_range_ptr", table._p, out._p, start_pos_buf._p, count, table.shape[1], table.itemsize, None)


# ---- [build-defined] LayerNorm + biased GEMV + GELU / residual in one launch (csrc/ops_lnlinear.hip) ------------------------
_LN_PLANS = {0: "generic", 1: "fp32_image", 2: "dtype_image"}
# K values the dispatcher has a specialised kernel for: none, K is a runtime argument on every path
LN_LINEAR_K_SPECIALIZATIONS: tuple = ()


def ln_linear_plan(m: int, k: int, n: int, dtype, *, norm: bool = True, aligned: bool = True) -> str:
    """[build-defined] The kernel an ln_linear call of this shape takes, decided on the host (needs no device): "fp32_image"
    (fast path, activations staged in LDS as fp32), "dtype_image" (fast path, no norm and an fp32 image beyond 64 KB: rows held
    in the dtype) or "generic" (k % 8 != 0, `aligned=False`: an operand off 16-byte alignment, a norm call beyond the LDS
    budget, or PGK_LN_LINEAR_GENERIC=1).  LN_LINEAR_K_SPECIALIZATIONS lists the K specialisations of the dispatcher (none)."""
    from pygpukit_amd import _hip
    from pygpukit_amd.core.dtypes import as_dtype

    plan = _hip.load().pgk_ln_linear_plan(int(m), int(k), int(n), as_dtype(dtype).code, int(bool(norm)), int(bool(aligned)))
    if plan < 0:
        raise ValueError(f"ln_linear_plan: invalid call m={m} (1..8) k={k} n={n} dtype={dtype}")
    return _LN_PLANS[plan]


def _ln_args(x: GPUArray, weight: GPUArray, bias, gamma, beta, name: str) -> tuple[int, int, int]:
    validate_float(x, name)
    if x.ndim != 2 or weight.ndim != 2 or x.shape[1] != weight.shape[1]:
        raise ValueError(f"{name}: x {x.shape} / weight {weight.shape} mismatch (x [m, k], weight [n, k])")
    m, k = x.shape
    n = weight.shape[0]
    if not 1 <= m <= 8:
        raise ValueError(f"{name}: m = {m} rows outside [1, 8] (more rows belong to matmul_nt)")
    if (gamma is None) != (beta is None):
        raise ValueError(f"{name}: gamma and beta come together (got beta without gamma, or gamma without beta)")
    for a, shape, what in ((weight, (n, k), "weight"), (bias, (n,), "bias"), (gamma, (k,), "gamma"), (beta, (k,), "beta")):
        if a is not None and (a.shape != shape or a.dtype != x.dtype):
            raise ValueError(f"{name}: {what} must be {shape} of {x.dtype}, got {a.shape} of {a.dtype}")
    return m, k, n


def _p(a):
    return a._p if a is not None else None


def ln_linear(x: GPUArray, weight: GPUArray, bias: GPUArray | None = None, *, gamma: GPUArray | None = None,
              beta: GPUArray | None = None, eps: float = 1e-5, activation: str | None = None, residual: GPUArray | None = None,
              out: GPUArray | None = None) -> GPUArray:
    """[build-defined] out[m, n] = act(LayerNorm(x[m, :]; gamma, beta, eps) . weight[n, :] + bias[n]) + residual[m, n] in ONE
    launch: x [m, k] with m = 1..8, weight [n, k].  gamma=None: no norm; activation None or "gelu" (the gelu op's function);
    residual may be `out` itself, x may not.  Statistics, the normalised row, the sum and the epilogue are fp32 with one rounding
    at the store.  The one-token kernel: measured faster than layernorm + matmul_nt + gelu / add at m = 1 and slower at m = 8."""
    m, k, n = _ln_args(x, weight, bias, gamma, beta, "ln_linear")
    if activation not in (None, "gelu"):
        raise ValueError(f"ln_linear: activation must be None or 'gelu', got {activation!r}")
    if residual is not None and (residual.shape != (m, n) or residual.dtype != x.dtype):
        raise ValueError(f"ln_linear: residual must be {(m, n)} of {x.dtype}, got {residual.shape} of {residual.dtype}")
    if out is not None and (out.shape != (m, n) or out.dtype != x.dtype):
        raise ValueError(f"ln_linear: out must be {(m, n)} of {x.dtype}, got {out.shape} of {out.dtype}")
    if out is not None and out.data_ptr() == x.data_ptr():
        raise ValueError("ln_linear: x may not alias out")
    o = out if out is not None else GPUArray((m, n), x.dtype)
    call("pgk_ln_linear", x._p, _p(gamma), _p(beta), weight._p, _p(bias), _p(residual), o._p, m, k, n, C.c_float(eps),
         1 if activation == "gelu" else 0, x.dtype.code, None)
    return o


def ln_linear_qkv_cache_ptr(x: GPUArray, qkv_weight: GPUArray, qkv_bias: GPUArray | None, q_out: GPUArray, k_cache: GPUArray,
                            v_cache: GPUArray, position_buf: GPUArray | None = None, *, gamma: GPUArray | None = None,
                            beta: GPUArray | None = None, eps: float = 1e-5, position: int | None = None) -> None:
    """[build-defined] ln_linear at m = 1 on the fused q | k | v weight [3 d, k], d = heads * head_dim, with the cache write in its
    epilogue: q -> q_out (d elements), k / v -> row `pos` of k_cache / v_cache [heads, max_seq, head_dim].  pos is read from the
    device int32 `position_buf` (clamped to the cache on the device), or is the host int `position`.  Bit-identical to ln_linear
    followed by two cache writes."""
    m, k, n = _ln_args(x, qkv_weight, qkv_bias, gamma, beta, "ln_linear_qkv_cache_ptr")
    if k_cache.ndim != 3 or v_cache.shape != k_cache.shape or k_cache.dtype != x.dtype or v_cache.dtype != x.dtype:
        raise ValueError(f"ln_linear_qkv_cache_ptr: caches must be equal [heads, max_seq, head_dim] of {x.dtype}, got {k_cache.shape} / {v_cache.shape}")
    heads, max_seq, head_dim = k_cache.shape
    if m != 1 or n != 3 * heads * head_dim:
        raise ValueError(f"ln_linear_qkv_cache_ptr: x must be [1, k] and qkv_weight [{3 * heads * head_dim}, k], got {x.shape} / {qkv_weight.shape}")
    if q_out.size != heads * head_dim or q_out.dtype != x.dtype:
        raise ValueError(f"ln_linear_qkv_cache_ptr: q_out must hold {heads * head_dim} elements of {x.dtype}")
    if (position_buf is None) == (position is None):
        raise ValueError("ln_linear_qkv_cache_ptr: give position_buf (device int32) or position (host int), not both")
    if position_buf is not None and position_buf.dtype != int32:
        raise ValueError("ln_linear_qkv_cache_ptr: position_buf must be int32")
    if position is not None and not 0 <= int(position) < max_seq:
        raise ValueError(f"ln_linear_qkv_cache_ptr: position {position} outside the cache of {max_seq} rows")
    call("pgk_ln_linear_qkv_cache", x._p, _p(gamma), _p(beta), qkv_weight._p, _p(qkv_bias), q_out._p, k_cache._p, v_cache._p, k, heads,
         head_dim, max_seq, C.c_float(eps), 0 if position is None else int(position), _p(position_buf), x.dtype.code, None)


def embed_token_position_ptr(token_table: GPUArray, position_table: GPUArray, out: GPUArray, state_buf: GPUArray) -> None:
    """[build-defined] out[:] = token_table[state[0]] + position_table[state[1]] (one fp32 add, one rounding); state_buf is a device
    int32 array of at least two elements, both indices are clamped to their table on the device."""
    if token_table.ndim != 2 or position_table.ndim != 2 or token_table.shape[1] != position_table.shape[1]:
        raise ValueError(f"embed_token_position_ptr: tables {token_table.shape} / {position_table.shape} mismatch")
    validate_float(token_table, "embed_token_position_ptr")
    validate_same_dtype(token_table, position_table, "embed_token_position_ptr")
    if out.size != token_table.shape[1] or out.dtype != token_table.dtype:
        raise ValueError(f"embed_token_position_ptr: out must hold {token_table.shape[1]} elements of {token_table.dtype}")
    if state_buf.dtype != int32 or state_buf.size < 2:
        raise ValueError("embed_token_position_ptr: state_buf must be int32 with at least two elements")
    call("pgk_embed_token_position", token_table._p, position_table._p, out._p, token_table.shape[1], token_table.shape[0],
         position_table.shape[0], state_buf._p, token_table.dtype.code, None)
