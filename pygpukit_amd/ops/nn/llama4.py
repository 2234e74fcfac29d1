"""Llama 4 attention ops (reference: src/pygpukit/ops/nn/llama4.py:16-283 -> native/ops/nn/llama4*).

    t(pos) = log1p(floor((pos + 1) / floor_scale)) * attn_scale + 1        (fp32, in that order)

l2norm, irope_scale_q and sdpa_irope keep the reference's signatures; sdpa_irope_strided is build-defined (the same op on
[S,H,D]-layout buffers), and so are the cached-decode ops llama4_qk_norm_cache_write and sdpa_irope_fixed_cache with
their _ptr forms (the reference has no cached Llama-4 path).  sdpa_irope runs on the MFMA flash-prefill kernel (csrc/ops_flash.hip) - float16 / bfloat16,
head_dim 64 or 128; the contract and the refused cases are in INTEGRATION.md."""

from __future__ import annotations

from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import bfloat16, float16, int32, int64
from pygpukit_amd.ops._common import call, check_out, validate_float
from pygpukit_amd.ops.nn.attention import _workspace          # the split-KV records, cached per (Hq, D, max_seq)

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


# ---- cached decode ---------------------------------------------------------------------------------------------------

def _check_prep(q: GPUArray, k: GPUArray, v: GPUArray, k_cache: GPUArray, v_cache: GPUArray, hq: int, hkv: int, d: int, name: str) -> int:
    _check_16bit(q, name)
    if any(a.dtype != q.dtype for a in (k, v, k_cache, v_cache)):
        raise ValueError(f"{name}: q, k, v and the caches must have the same dtype")
    if d not in (64, 128):
        raise ValueError(f"{name}: head_dim must be 64 or 128, got {d}")
    if hq <= 0 or hkv <= 0 or hq % hkv != 0:
        raise ValueError(f"{name}: n_heads mismatch (Hq={hq}, Hkv={hkv})")
    if q.ndim != 2 or q.shape[0] < 1 or q.shape[1] != hq * d:
        raise ValueError(f"{name}: q must be [S, {hq * d}] with S >= 1, got {q.shape}")
    seq = q.shape[0]
    if k.shape != (seq, hkv * d) or v.shape != (seq, hkv * d):
        raise ValueError(f"{name}: k {k.shape} / v {v.shape} must be {(seq, hkv * d)}")
    if k_cache.ndim != 3 or k_cache.shape[0] != hkv or k_cache.shape[2] != d or v_cache.shape != k_cache.shape:
        raise ValueError(f"{name}: caches must both be [{hkv}, max_seq, {d}], got {k_cache.shape} / {v_cache.shape}")
    return seq


def llama4_qk_norm_cache_write(q: GPUArray, k: GPUArray, v: GPUArray, k_cache: GPUArray, v_cache: GPUArray, position: int, *,
                               num_heads: int, num_kv_heads: int, head_dim: int, eps: float, qk_norm: bool = True) -> None:
    """[build-defined] One launch over the projection buffers q [S, Hq*D], k / v [S, Hkv*D]: l2norm of every Q head in
    place, l2norm of every K head on its way to k_cache[h, position + s] (k itself is left as projected), V copied to
    v_cache[h, position + s]; caches [Hkv, max_seq, D].  Bit-identical to l2norm + kv_cache_prefill_gqa.  With
    qk_norm=False q is untouched and K is copied."""
    name = "llama4_qk_norm_cache_write"
    seq = _check_prep(q, k, v, k_cache, v_cache, num_heads, num_kv_heads, head_dim, name)
    if position < 0 or position + seq > k_cache.shape[1]:
        raise ValueError(f"{name}: rows {position}..{position + seq} outside cache of {k_cache.shape[1]} rows")
    call("pgk_llama4_qk_norm_cache_write", q._p, k._p, v._p, k_cache._p, v_cache._p, seq, num_heads, num_kv_heads, k_cache.shape[1],
         head_dim, float(eps), int(bool(qk_norm)), int(position), None, q.dtype.code, None)


def llama4_qk_norm_cache_write_ptr(q: GPUArray, k: GPUArray, v: GPUArray, k_cache: GPUArray, v_cache: GPUArray, position_buf: GPUArray, *,
                                   num_heads: int, num_kv_heads: int, head_dim: int, eps: float, qk_norm: bool = True) -> None:
    """As above with the first row's position read from a device int32 (graph replay).  Rows that would fall outside
    the cache are not written."""
    name = "llama4_qk_norm_cache_write_ptr"
    seq = _check_prep(q, k, v, k_cache, v_cache, num_heads, num_kv_heads, head_dim, name)
    if position_buf.dtype != int32 or position_buf.size < 1:
        raise ValueError(f"{name}: position_buf must be int32 with at least one element")
    call("pgk_llama4_qk_norm_cache_write", q._p, k._p, v._p, k_cache._p, v_cache._p, seq, num_heads, num_kv_heads, k_cache.shape[1],
         head_dim, float(eps), int(bool(qk_norm)), 0, position_buf._p, q.dtype.code, None)


def _check_fixed_cache(Q: GPUArray, K: GPUArray, V: GPUArray, out: GPUArray, floor_scale: float, name: str):
    _check_16bit(Q, name)
    if Q.ndim != 3 or K.ndim != 3 or V.ndim != 3:
        raise ValueError(f"{name} expects 3D Q [Hq, 1, D] and caches [Hkv, max_seq, D]")
    if Q.dtype != K.dtype or Q.dtype != V.dtype or out.dtype != Q.dtype:
        raise ValueError(f"{name}: Q, the caches and out must have the same dtype")
    hq, q_len, d = Q.shape
    hkv, max_seq = K.shape[0], K.shape[1]
    if q_len != 1:
        raise ValueError(f"{name}: q_len must be 1, got {q_len}")
    if d not in (64, 128):
        raise ValueError(f"{name}: head_dim must be 64 or 128, got {d}")
    if K.shape != V.shape or K.shape[2] != d or max_seq < 1:
        raise ValueError(f"{name}: caches {K.shape} / {V.shape} do not fit Q {Q.shape}")
    if hkv <= 0 or hq % hkv != 0:
        raise ValueError(f"{name}: n_heads mismatch (Hq={hq}, Hkv={hkv})")
    if out.shape != Q.shape:
        raise ValueError(f"{name}: out shape {out.shape} does not match Q {Q.shape}")
    if not floor_scale > 0:
        raise ValueError(f"{name}: floor_scale must be positive, got {floor_scale}")
    return hq, hkv, max_seq, d


def sdpa_irope_fixed_cache(Q: GPUArray, K_cache: GPUArray, V_cache: GPUArray, out: GPUArray, position: int, attn_scale: float = 0.1,
                           floor_scale: float = 8192.0) -> None:
    """[build-defined] The query row Q [Hq, 1, D] at `position` over rows 0 .. position of the fixed caches
    [Hkv, max_seq, D], written into `out`: sdpa_irope(Q, cache[:, :position+1], positions=[position],
    causal_offset=position) as split-KV flash-decoding; the temperature stays in fp32."""
    hq, hkv, max_seq, d = _check_fixed_cache(Q, K_cache, V_cache, out, floor_scale, "sdpa_irope_fixed_cache")
    if not 0 <= position < max_seq:
        raise ValueError(f"sdpa_irope_fixed_cache: position {position} outside cache of {max_seq} rows")
    call("pgk_sdpa_irope_fixed_cache", Q._p, K_cache._p, V_cache._p, out._p, hq, hkv, max_seq, d, float(attn_scale), float(floor_scale),
         int(position), None, _workspace(hq, d, max_seq)._p, Q.dtype.code, None)


def sdpa_irope_fixed_cache_ptr(Q: GPUArray, K_cache: GPUArray, V_cache: GPUArray, out: GPUArray, position_buf: GPUArray,
                               attn_scale: float = 0.1, floor_scale: float = 8192.0) -> None:
    """As above with the position read from a device int32 (graph replay); the context is clamped to the cache."""
    hq, hkv, max_seq, d = _check_fixed_cache(Q, K_cache, V_cache, out, floor_scale, "sdpa_irope_fixed_cache_ptr")
    if position_buf.dtype != int32 or position_buf.size < 1:
        raise ValueError("sdpa_irope_fixed_cache_ptr: position_buf must be int32 with at least one element")
    call("pgk_sdpa_irope_fixed_cache", Q._p, K_cache._p, V_cache._p, out._p, hq, hkv, max_seq, d, float(attn_scale), float(floor_scale),
         0, position_buf._p, _workspace(hq, d, max_seq)._p, Q.dtype.code, None)


__all__ = ["l2norm", "irope_scale_q", "sdpa_irope", "sdpa_irope_strided", "llama4_qk_norm_cache_write",
           "llama4_qk_norm_cache_write_ptr", "sdpa_irope_fixed_cache", "sdpa_irope_fixed_cache_ptr"]
