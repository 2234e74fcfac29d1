"""Adaptive LayerNorm for diffusion transformers (reference: src/pygpukit/diffusion/ops/adaln.py and the native-only ops of
native/ops/nn/diffusion.inl).  Every function here is one launch of pgk_adaln_fused (csrc/ops_diffusion.hip): LayerNorm without
gamma / beta on fp32 rows, modulated by per-sample vectors, optionally behind a gated residual.

  adaln, adaln_zero                the reference's ops: (1 + scale) * LN(x) + shift, and residual + gate * that
  layer_norm_simple, modulate,
  gated_residual                   the reference's native-only ops
  gated_residual_adaln             [build-defined] sum = residual + gate * value; y = LN(sum) * (1 + scale) + shift in ONE pass:
                                   the end of one DiT sub-layer and the modulated input of the next
A modulation vector (gate / scale / shift) is given as a GPUArray [B, D], a GPUArray [D] shared by the batch, or a `Modulation`
(table [D] + rows of a larger array, read in place - PixArt's scale_shift_table [6, D] and adaln_single output [B, 6, D])."""

from __future__ import annotations

from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import float32
from pygpukit_amd.ops._common import call, check_out, validate_float


class Modulation:
    """table[offset_t : offset_t + D] + vector[offset_v + b * stride : ... + D] for batch element b; either part may be None.
    `stride` is in elements (None: D for a [B, D] vector; 0: one vector for every batch element).  Nothing is copied or summed on
    the host: the kernel reads both parts in place."""

    __slots__ = ("table", "table_offset", "vector", "vector_offset", "stride")

    def __init__(self, table: "GPUArray | None" = None, vector: "GPUArray | None" = None, *, table_offset: int = 0,
                 vector_offset: int = 0, stride: "int | None" = None):
        self.table, self.table_offset = table, int(table_offset)
        self.vector, self.vector_offset, self.stride = vector, int(vector_offset), stride


def _as_mod(m, name: str) -> "Modulation | None":
    if m is None or isinstance(m, Modulation):
        return m
    if not isinstance(m, GPUArray) or m.ndim not in (1, 2):
        raise ValueError(f"{name} must be a GPUArray [B, D] or [D], or a Modulation")
    return Modulation(table=m) if m.ndim == 1 else Modulation(vector=m)


def _resolve(mods, batch: int, features: int, row_dtype, op: str):
    """-> (vector dtype, [(table ptr, vector ptr, stride)] * 3) after bounds checks: every read stays inside its array."""
    vec_dt, out = None, []
    for label, m in mods:
        if m is None or (m.table is None and m.vector is None):
            out.append((None, None, 0))
            continue
        tp = vp = None
        stride = 0
        for part in (m.table, m.vector):
            if part is None:
                continue
            if part.dtype != row_dtype and part.dtype != float32:
                raise ValueError(f"{op}: {label} must be {row_dtype.name} or float32, got {part.dtype.name}")
            if vec_dt is not None and part.dtype != vec_dt:
                raise ValueError(f"{op}: every modulation vector must share one dtype, got {vec_dt.name} and {part.dtype.name}")
            vec_dt = part.dtype
        if m.table is not None:
            if m.table_offset < 0 or m.table_offset + features > m.table.size:
                raise ValueError(f"{op}: {label} table of {m.table.size} elements has no {features} at offset {m.table_offset}")
            tp = m.table.data_ptr() + m.table_offset * m.table.itemsize
        if m.vector is not None:
            stride = features if m.stride is None else int(m.stride)
            if stride < 0 or m.vector_offset < 0 or m.vector_offset + (batch - 1) * stride + features > m.vector.size:
                raise ValueError(f"{op}: {label} vector of {m.vector.size} elements has no {batch} rows of {features} at offset "
                                 f"{m.vector_offset}, stride {stride}")
            vp = m.vector.data_ptr() + m.vector_offset * m.vector.itemsize
        out.append((tp, vp, stride))
    return vec_dt, out


def _launch(op: str, x: GPUArray, residual, sum_out, y, gate, scale, shift, eps: float, norm: bool, mode: int) -> None:
    validate_float(x, op)
    if x.ndim != 3:
        raise ValueError(f"{op} expects 3D input [B, N, D], got {x.ndim}D")
    B, N, D = x.shape
    for label, a in (("residual", residual), ("sum_out", sum_out), ("out", y)):
        if a is not None and (a.shape != x.shape or a.dtype != x.dtype):
            raise ValueError(f"{op}: {label} must be {x.shape} {x.dtype.name}, got {a.shape} {a.dtype.name}")
    mods = [(label, _as_mod(m, f"{op}: {label}")) for label, m in (("gate", gate), ("scale", scale), ("shift", shift))]
    for label, m in mods:
        if m is not None and m.vector is not None and m.vector.ndim == 2 and m.stride is None and m.vector_offset == 0 \
                and m.vector.shape != (B, D):
            raise ValueError(f"{op}: {label} must be [{B}, {D}], got {m.vector.shape}")
        if m is not None and m.table is not None and m.table.ndim == 1 and m.table_offset == 0 and m.table.shape != (D,):
            raise ValueError(f"{op}: {label} must be [{D}], got {m.table.shape}")
    if B == 0 or N == 0:
        return
    vec_dt, ((gt, gv, gs), (st, sv, ss), (ht, hv, hs)) = _resolve(mods, B, D, x.dtype, op)
    call("pgk_adaln_fused", x._p, residual._p if residual is not None else None, sum_out._p if sum_out is not None else None,
         y._p if y is not None else None, gt, gv, gs, st, sv, ss, ht, hv, hs, B, N, D, float(eps), int(bool(norm)), mode,
         x.dtype.code, (vec_dt or x.dtype).code, None)


def adaln(x: GPUArray, scale, shift, eps: float = 1e-5, *, out: GPUArray | None = None) -> GPUArray:
    """(1 + scale) * LayerNorm(x) + shift: x [B, N, D], scale / shift [B, D]."""
    if x.ndim != 3:
        raise ValueError(f"adaln expects 3D input [B, N, D], got {x.ndim}D")
    if scale is None or shift is None:
        raise ValueError("adaln: scale and shift are required")
    o = check_out(out, x.shape, x.dtype, "adaln")
    _launch("adaln", x, None, None, o, None, scale, shift, eps, True, 0)
    return o


def adaln_zero(x: GPUArray, scale, shift, gate, residual: GPUArray, eps: float = 1e-5, *, out: GPUArray | None = None) -> GPUArray:
    """residual + gate * ((1 + scale) * LayerNorm(x) + shift), the reference's AdaLN-Zero."""
    if x.ndim != 3:
        raise ValueError(f"adaln_zero expects 3D input [B, N, D], got {x.ndim}D")
    if scale is None or shift is None or gate is None or residual is None:
        raise ValueError("adaln_zero: scale, shift, gate and residual are required")
    o = check_out(out, x.shape, x.dtype, "adaln_zero")
    _launch("adaln_zero", x, residual, None, o, gate, scale, shift, eps, True, 1)
    return o


def layer_norm_simple(x: GPUArray, eps: float = 1e-5, *, out: GPUArray | None = None) -> GPUArray:
    """LayerNorm over the last axis without gamma / beta."""
    o = check_out(out, x.shape, x.dtype, "layer_norm_simple")
    _launch("layer_norm_simple", x, None, None, o, None, None, None, eps, True, 0)
    return o


def modulate(x: GPUArray, scale, shift, *, out: GPUArray | None = None) -> GPUArray:
    """x * (1 + scale) + shift."""
    o = check_out(out, x.shape, x.dtype, "modulate")
    _launch("modulate", x, None, None, o, None, scale, shift, 0.0, False, 0)
    return o


def gated_residual(residual: GPUArray, gate, value: GPUArray, *, out: GPUArray | None = None) -> GPUArray:
    """residual + gate * value; `out` may be `residual`."""
    o = check_out(out, value.shape, value.dtype, "gated_residual")
    _launch("gated_residual", value, residual, o, None, gate, None, None, 0.0, False, 0)
    return o


def gated_residual_adaln(value: GPUArray, residual: "GPUArray | None", gate, scale, shift, eps: float = 1e-5, *, norm: bool = True,
                         sum_out: GPUArray | None = None, out: GPUArray | None = None) -> "tuple[GPUArray | None, GPUArray]":
    """[build-defined] One pass: sum = residual + gate * value (value when residual is None; gate None = 1), rounded once into
    `sum_out`, and y = (LN(sum) if norm else sum) * (1 + scale) + shift from the UNROUNDED fp32 sum, rounded once into `out`.
    `sum_out` may be `residual` and `out` may be `value`.  Returns (sum, y); sum is None when there is no residual."""
    if residual is None:
        if gate is not None or sum_out is not None:
            raise ValueError("gated_residual_adaln: gate and sum_out need a residual")
        s = None
    else:
        s = check_out(sum_out, value.shape, value.dtype, "gated_residual_adaln")
    y = check_out(out, value.shape, value.dtype, "gated_residual_adaln")
    _launch("gated_residual_adaln", value, residual, s, y, gate, scale, shift, eps, norm, 0)
    return s, y


def adaln_plan(features: int, dtype, aligned: bool = True) -> str:
    """"adaln_wave" (a wave per row, the row in registers) or "adaln_block" (a 256-thread block per row, scalar accesses), from the
    function the launcher calls; needs no device.  aligned=False: a row pointer, table, vector or vector stride off 16 bytes."""
    from pygpukit_amd import _hip
    from pygpukit_amd.core.dtypes import as_dtype

    lib = _hip.load()
    plan = lib.pgk_adaln_plan(int(features), as_dtype(dtype).code, int(bool(aligned)))
    if plan is None:
        msg = lib.pgk_last_error()
        raise ValueError(msg.decode(errors="replace") if msg else f"adaln_plan: invalid call features={features} dtype={dtype}")
    return plan.decode()


def modulation(conditioning: GPUArray, linear_weight: GPUArray, linear_bias: GPUArray, num_outputs: int = 6) -> list[GPUArray]:
    """conditioning [B, D] -> num_outputs modulation vectors through one matmul_nt on weight [num_outputs * D', D].  For B == 1 the
    results are zero-copy views [1, D'] of the projection; for B > 1 they are `Modulation`s over it (offset i * D', stride
    num_outputs * D'), which every op of this module accepts - still no copy."""
    from pygpukit_amd.ops.matmul import matmul_nt

    if conditioning.ndim != 2:
        raise ValueError(f"modulation expects conditioning [B, D], got {conditioning.shape}")
    if num_outputs < 1 or linear_weight.shape[0] % num_outputs:
        raise ValueError(f"modulation: {linear_weight.shape[0]} outputs do not split into {num_outputs}")
    proj = matmul_nt(conditioning, linear_weight, linear_bias)
    B, d = conditioning.shape[0], linear_weight.shape[0] // num_outputs
    if B == 1:
        return [proj._view(i * d, (1, d)) for i in range(num_outputs)]
    return [Modulation(vector=proj, vector_offset=i * d, stride=num_outputs * d) for i in range(num_outputs)]


__all__ = ["adaln", "adaln_zero", "modulation", "layer_norm_simple", "modulate", "gated_residual", "gated_residual_adaln",
           "adaln_plan", "Modulation"]
