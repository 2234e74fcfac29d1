"""Llama 4 attention ops (reference: src/pygpukit/ops/nn/llama4.py:16-283 -> native/ops/nn/llama4*).

    t(pos) = log1p(floor((pos + 1) / floor_scale)) * attn_scale + 1        (fp32, in that order)

l2norm, irope_scale_q and sdpa_irope keep the reference's signatures; sdpa_irope_strided is build-defined (the same op on
[S,H,D]-layout buffers).  sdpa_irope runs on the MFMA flash-prefill kernel (csrc/ops_flash.hip) - float16 / bfloat16,
head_dim 64 or 128; the contract and the refused cases are in INTEGRATION.md."""

from __future__ import annotations

from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import bfloat16, float16, int32, int64
from pygpukit_amd.ops._common import call, check_out, validate_float

_POS_DTYPES = (int64, int32)


def l2norm(input: GPUArray, eps: float = 1e-6, *, out: GPUArray | None = None) -> GPUArray:
    """x * rsqrt(mean(x^2) + eps) over the last dimension, no gamma (Llama4TextL2Norm); `out` may be `input`."""
    validate_float(input, "l2norm")
    if input.ndim < 1:
        raise ValueError(f"l2norm expects at least 1D input, got {input.ndim}D")
    if out is not None:
        if out.shape != input.shape:
            raise ValueError(f"out shape {out.shape} does not match input shape {input.shape}")
        if out.dtype != input.dtype:
            raise ValueError(f"out dtype {out.dtype} does not match input dtype {input.dtype}")
    o = check_out(out, input.shape, input.dtype, "l2norm")
    features = input.shape[-1]
    if features < 1:
        raise ValueError("l2norm: the last dimension is empty")
    call("pgk_l2norm", input._p, o._p, input.size // features, features, float(eps), input.dtype.code, None)
    return o


def _check_positions(positions: GPUArray, n: int, name: str) -> None:
    if positions.dtype not in _POS_DTYPES:
        raise ValueError(f"{name}: positions must be int64 or int32, got {positions.dtype}")
    if positions.ndim != 1 or positions.shape[0] != n:
        raise ValueError(f"{name}: positions must have shape ({n},), got {positions.shape}")


def _check_16bit(a: GPUArray, name: str) -> None:
    validate_float(a, name)
    if a.dtype not in (bfloat16, float16):
        raise ValueError(f"{name} requires float16/bfloat16, got {a.dtype}")


def irope_scale_q(Q: GPUArray, positions: GPUArray, attn_scale: float = 0.1, floor_scale: float = 8192.0) -> GPUArray:
    """Q [seq_len, num_heads, head_dim] * t(positions[seq]) - the temperature scaling on its own (fp32 multiply, one
    rounding).  sdpa_irope applies it inside the attention; do not use both."""
    validate_float(Q, "irope_scale_q")
    if Q.ndim != 3:
        raise ValueError(f"irope_scale_q expects 3D Q [seq_len, num_heads, head_dim], got {Q.ndim}D")
    _check_16bit(Q, "irope_scale_q")
    _check_positions(positions, Q.shape[0], "irope_scale_q")
    if not floor_scale > 0:
        raise ValueError(f"irope_scale_q: floor_scale must be positive, got {floor_scale}")
    o = GPUArray(Q.shape, Q.dtype)
    call("pgk_irope_scale_q", Q._p, positions._p, o._p, Q.shape[0], Q.shape[1], Q.shape[2], float(attn_scale), float(floor_scale),
         positions.dtype.code, Q.dtype.code, None)
    return o


def _check_irope(q: GPUArray, k: GPUArray, v: GPUArray, out: GPUArray | None, positions: GPUArray, hq: int, hkv: int, q_len: int,
                 kv_len: int, d: int, floor_scale: float, causal_offset: int, name: str) -> None:
    _check_16bit(q, name)
    if q.dtype != k.dtype or q.dtype != v.dtype:
        raise ValueError(f"{name}: Q/K/V must have same dtype")
    if out is not None and out.dtype != q.dtype:
        raise ValueError(f"{name}: out must have same dtype as Q")
    if d not in (64, 128):
        raise ValueError(f"{name}: head_dim must be 64 or 128, got {d}")
    if hq <= 0 or hkv <= 0 or hq % hkv != 0:
        raise ValueError(f"{name}: n_heads mismatch (Hq={hq}, Hkv={hkv})")
    if q_len < 1 or kv_len < 1:
        raise ValueError(f"{name}: needs q_len >= 1 and kv_len >= 1, got q_len {q_len}, kv_len {kv_len}")
    if causal_offset < 0:
        raise ValueError(f"{name}: causal_offset must be >= 0, got {causal_offset} (row 0 would see no key)")
    if not floor_scale > 0:
        raise ValueError(f"{name}: floor_scale must be positive, got {floor_scale}")
    _check_positions(positions, q_len, name)


def sdpa_irope(Q: GPUArray, K: GPUArray, V: GPUArray, positions: GPUArray, attn_scale: float = 0.1, floor_scale: float = 8192.0,
               causal_offset: int = 0) -> GPUArray:
    """softmax(Q K^T * t(positions[i]) / sqrt(head_dim) + mask) V with Q [Hq, q_len, D], K / V [Hkv, kv_len, D]
    (un-expanded GQA: kv head = q head // (Hq/Hkv)) and positions [q_len]; query row i sees kv j <= i + causal_offset."""
    validate_float(Q, "sdpa_irope")
    if Q.ndim != 3 or K.ndim != 3 or V.ndim != 3:
        raise ValueError("sdpa_irope expects 3D Q, K, V [heads, seq, head_dim]")
    if Q.dtype != K.dtype or Q.dtype != V.dtype:
        raise ValueError("sdpa_irope: Q/K/V must have same dtype")
    hq, q_len, d = Q.shape
    hkv, kv_len = K.shape[0], K.shape[1]
    if K.shape != V.shape or K.shape[2] != d:
        raise ValueError(f"sdpa_irope: K {K.shape} / V {V.shape} do not fit Q {Q.shape}")
    _check_irope(Q, K, V, None, positions, hq, hkv, q_len, kv_len, d, floor_scale, int(causal_offset), "sdpa_irope")
    o = GPUArray((hq, q_len, d), Q.dtype)
    call("pgk_sdpa_irope", Q._p, K._p, V._p, positions._p, o._p, hq, hkv, q_len, kv_len, d, float(attn_scale), float(floor_scale),
         int(causal_offset), q_len * d, d, kv_len * d, d, q_len * d, d, positions.dtype.code, Q.dtype.code, None)
    return o


def sdpa_irope_strided(q: GPUArray, k: GPUArray, v: GPUArray, positions: GPUArray, out: GPUArray, hq: int, hkv: int, q_len: int,
                       kv_len: int, d: int, q_strides, kv_strides, o_strides, attn_scale: float = 0.1, floor_scale: float = 8192.0,
                       causal_offset: int = 0) -> None:
    """[build-defined] sdpa_irope on [S,H,D]-layout (or any head/row-strided) buffers, written into `out`: strides are
    (head, row) in elements, multiples of 8."""
    _check_irope(q, k, v, out, positions, hq, hkv, q_len, kv_len, d, floor_scale, int(causal_offset), "sdpa_irope_strided")
    if any(int(x) % 8 or int(x) < 0 for x in (*q_strides, *kv_strides, *o_strides)):
        raise ValueError("sdpa_irope_strided: strides must be non-negative multiples of 8 elements")
    call("pgk_sdpa_irope", q._p, k._p, v._p, positions._p, out._p, hq, hkv, q_len, kv_len, d, float(attn_scale), float(floor_scale),
         int(causal_offset), q_strides[0], q_strides[1], kv_strides[0], kv_strides[1], o_strides[0], o_strides[1],
         positions.dtype.code, q.dtype.code, None)


__all__ = ["l2norm", "irope_scale_q", "sdpa_irope", "sdpa_irope_strided"]
