"""[build-defined] FLUX row ops (csrc/ops_flux.hip); the reference composes each from several ops and host round trips
(src/pygpukit/diffusion/models/flux/attention.py, blocks.py, pipeline.py, scheduler.py).

  flux_qk_norm_rope     per-head RMSNorm of Q and K with learned weights + interleaved-pair RoPE from [S, D] fp32 tables, in
                        place, one launch; rows below `split` of every sequence use one weight pair, the others a second
  flux_gelu_pack        gelu(x [rows, cols]) written into columns of a wider destination
  flux_unpack_latents   [B, h w, C 4] with columns (c, ph, pw) -> [B, C, 2h, 2w]
  flow_euler_step       sample_f32 += dt * v
Q and K are given as flat views starting at the first element of row 0, head 0: the op addresses row r, head h at
r * row_stride + h * head_stride and checks that the last element it touches lies inside the array."""

from __future__ import annotations

from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import as_dtype, float32
from pygpukit_amd.ops._common import call, check_out, validate_float


def flux_qk_norm_rope(q: GPUArray, k: GPUArray, cos: GPUArray, sin: GPUArray, wq: GPUArray, wk: GPUArray, *, batch: int, seq: int,
                      heads: int, head_dim: int, row_stride: int, head_stride: "int | None" = None, split: "int | None" = None,
                      wq_b: "GPUArray | None" = None, wk_b: "GPUArray | None" = None, eps: float = 1e-6) -> None:
    """In place on q and k (any shape; element 0 is row 0, head 0).  wq / wk serve positions p < split, wq_b / wk_b the others;
    split None = seq (one weight pair).  cos / sin: [seq, head_dim] float32, indexed by the position inside the sequence."""
    op = "flux_qk_norm_rope"
    validate_float(q, op)
    if k.dtype != q.dtype:
        raise ValueError(f"{op}: q is {q.dtype.name} and k is {k.dtype.name}")
    batch, seq, heads, head_dim, row_stride = int(batch), int(seq), int(heads), int(head_dim), int(row_stride)
    head_stride = head_dim if head_stride is None else int(head_stride)
    split = seq if split is None else int(split)
    if batch < 0 or seq < 0 or heads < 1 or head_dim < 1:
        raise ValueError(f"{op}: bad shape batch={batch} seq={seq} heads={heads} head_dim={head_dim}")
    if head_dim % 2:
        raise ValueError(f"{op}: head_dim {head_dim} must be even (rotation pairs)")
    if not 0 <= split <= seq:
        raise ValueError(f"{op}: split {split} outside [0, {seq}]")
    if row_stride < 0 or head_stride < 0:
        raise ValueError(f"{op}: negative stride")
    rows = batch * seq
    if rows == 0:
        return
    last = (rows - 1) * row_stride + (heads - 1) * head_stride + head_dim
    for name, a in (("q", q), ("k", k)):
        if last > a.size:
            raise ValueError(f"{op}: {name} of {a.size} elements has no {rows} rows of {heads} heads at strides {row_stride}, {head_stride}")
    for name, t in (("cos", cos), ("sin", sin)):
        if t.dtype != float32 or t.size < seq * head_dim or (t.ndim == 2 and t.shape[1] != head_dim):
            raise ValueError(f"{op}: {name} must be float32 [{seq}, {head_dim}], got {t.shape} {t.dtype.name}")
    need_a, need_b = split > 0, split < seq
    w_dt = None
    for name, w, needed in (("wq", wq, need_a), ("wk", wk, need_a), ("wq_b", wq_b, need_b), ("wk_b", wk_b, need_b)):
        if w is None:
            if needed:
                raise ValueError(f"{op}: {name} is required for split {split} of {seq}")
            continue
        if w.size < head_dim or (w.dtype != q.dtype and w.dtype != float32):
            raise ValueError(f"{op}: {name} must be [{head_dim}] in {q.dtype.name} or float32, got {w.shape} {w.dtype.name}")
        if w_dt is not None and w.dtype != w_dt:
            raise ValueError(f"{op}: every norm weight must share one dtype, got {w_dt.name} and {w.dtype.name}")
        w_dt = w.dtype
    call("pgk_flux_qk_norm_rope", q._p, k._p, row_stride, head_stride, wq._p if wq is not None else None,
         wk._p if wk is not None else None, wq_b._p if wq_b is not None else None, wk_b._p if wk_b is not None else None, cos._p, sin._p,
         batch, seq, split, heads, head_dim, float(eps), q.dtype.code, w_dt.code, None)


def flux_qk_norm_rope_plan(head_dim: int, dtype, aligned: bool = True) -> str:
    """"flux_qk_norm_rope_vec" (head_dim 64 / 128, everything on 16 bytes) or "flux_qk_norm_rope_scalar"; needs no device."""
    from pygpukit_amd import _hip

    lib = _hip.load()
    plan = lib.pgk_flux_qk_norm_rope_plan(int(head_dim), as_dtype(dtype).code, int(bool(aligned)))
    if plan is None:
        msg = lib.pgk_last_error()
        raise ValueError(msg.decode(errors="replace") if msg else f"flux_qk_norm_rope_plan: invalid call head_dim={head_dim} dtype={dtype}")
    return plan.decode()


def flux_gelu_pack(x: GPUArray, out: GPUArray, column: int = 0) -> GPUArray:
    """out[r, column + c] = gelu(x[r, c]) for x [rows, cols] and out [rows, width]; the other columns of out are not touched."""
    op = "flux_gelu_pack"
    validate_float(x, op)
    if x.ndim != 2 or out.ndim != 2 or out.dtype != x.dtype or out.shape[0] != x.shape[0]:
        raise ValueError(f"{op}: x [rows, cols] and out [rows, width] of one dtype, got {x.shape} {x.dtype.name} and {out.shape} {out.dtype.name}")
    rows, cols = x.shape
    column = int(column)
    if column < 0 or column + cols > out.shape[1]:
        raise ValueError(f"{op}: columns {column}..{column + cols} do not fit a width of {out.shape[1]}")
    if rows and cols:
        dst = out._view(column, (out.size - column,))
        call("pgk_flux_gelu_pack", x._p, dst._p, rows, cols, out.shape[1], x.dtype.code, None)
    return out


def flux_unpack_latents(x: GPUArray, h: int, w: int, *, out: "GPUArray | None" = None) -> GPUArray:
    """[B, h * w, C * 4] with columns (c, ph, pw) -> [B, C, 2h, 2w] (the reference's FluxPipeline._unpack_latents)."""
    op = "flux_unpack_latents"
    h, w = int(h), int(w)
    if x.ndim != 3 or x.itemsize not in (2, 4) or h < 1 or w < 1 or x.shape[1] != h * w or x.shape[2] % 4:
        raise ValueError(f"{op} expects [B, {h * w}, C * 4] of 2- or 4-byte elements, got {x.shape} {x.dtype.name}")
    B, C = x.shape[0], x.shape[2] // 4
    o = check_out(out, (B, C, 2 * h, 2 * w), x.dtype, op)
    call("pgk_flux_unpack_latents", x._p, o._p, B, C, h, w, x.dtype.code, None)
    return o


def flow_euler_step(sample: GPUArray, model_output: GPUArray, dt: float) -> GPUArray:
    """sample += dt * model_output, in place on the float32 sample; model_output in any float dtype."""
    op = "flow_euler_step"
    validate_float(model_output, op)
    if sample.dtype != float32 or sample.size != model_output.size:
        raise ValueError(f"{op}: sample must be float32 with {model_output.size} elements, got {sample.shape} {sample.dtype.name}")
    call("pgk_flow_euler_step", sample._p, model_output._p, sample.size, float(dt), model_output.dtype.code, None)
    return sample


__all__ = ["flux_qk_norm_rope", "flux_qk_norm_rope_plan", "flux_gelu_pack", "flux_unpack_latents", "flow_euler_step"]
