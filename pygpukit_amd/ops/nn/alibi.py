"""[build-defined] Causal attention with the ALiBi bias applied inside the attention kernels.

    out[h, i] = softmax_j(q[h, i] . k[h // rep, j] * scale - slopes[h] * (kv_len - q_len + i - j), over j <= kv_len - q_len + i) . v[h // rep]

The reference offers ALiBi only as a materialised [H, S, S] bias (alibi_compute_bias) or an in-place add on materialised
scores (alibi_add_bias); attention here never holds the scores in memory, so the bias enters the MFMA flash-prefill kernel
(csrc/ops_flash.hip, FlashAlibi) and the split-KV decode walk (csrc/ops_posenc.hip).  float16 / bfloat16, head_dim 64 or
128, slopes float32 with one element per QUERY head; scale <= 0 means 1 / sqrt(head_dim).  Contract: INTEGRATION.md."""

from __future__ import annotations

from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import bfloat16, float16, float32, int32
from pygpukit_amd.ops._common import call, check_out, validate_float
from pygpukit_amd.ops.nn.attention import _workspace          # the split-KV records, cached per (Hq, D, max_seq)


def _check_alibi(q: GPUArray, k: GPUArray, v: GPUArray, out: GPUArray | None, slopes: GPUArray, hq: int, hkv: int, q_len: int,
                 kv_len: int, d: int, name: str) -> None:
    validate_float(q, name)
    if q.dtype not in (bfloat16, float16):
        raise ValueError(f"{name} requires float16/bfloat16, got {q.dtype}")
    if q.dtype != k.dtype or q.dtype != v.dtype:
        raise ValueError(f"{name}: Q/K/V must have same dtype")
    if out is not None and out.dtype != q.dtype:
        raise ValueError(f"{name}: out must have same dtype as Q")
    if d not in (64, 128):
        raise ValueError(f"{name}: head_dim must be 64 or 128, got {d}")
    if hq <= 0 or hkv <= 0 or hq % hkv != 0:
        raise ValueError(f"{name}: n_heads mismatch (Hq={hq}, Hkv={hkv})")
    if q_len < 1 or kv_len < q_len:
        raise ValueError(f"{name}: needs kv_len >= q_len >= 1, got q_len {q_len}, kv_len {kv_len}")
    if slopes.dtype != float32:
        raise ValueError(f"{name}: slopes must be float32, got {slopes.dtype}")
    if slopes.size != hq:
        raise ValueError(f"{name}: slopes must have {hq} elements (one per query head), got shape {slopes.shape}")


def sdpa_alibi(Q: GPUArray, K: GPUArray, V: GPUArray, slopes: GPUArray, scale: float = 0.0, *, out: GPUArray | None = None) -> GPUArray:
    """Q [Hq, q_len, D], K / V [Hkv, kv_len, D] (un-expanded GQA), slopes [Hq]: causal attention whose scores carry
    -slopes[h] * distance; equals attention with alibi_compute_bias added to the scaled scores."""
    if Q.ndim != 3 or K.ndim != 3 or V.ndim != 3:
        raise ValueError("sdpa_alibi expects 3D Q, K, V [heads, seq, head_dim]")
    hq, q_len, d = Q.shape
    hkv, kv_len = K.shape[0], K.shape[1]
    if K.shape != V.shape or K.shape[2] != d:
        raise ValueError(f"sdpa_alibi: K {K.shape} / V {V.shape} do not fit Q {Q.shape}")
    _check_alibi(Q, K, V, out, slopes, hq, hkv, q_len, kv_len, d, "sdpa_alibi")
    o = check_out(out, (hq, q_len, d), Q.dtype, "sdpa_alibi")
    call("pgk_sdpa_alibi", Q._p, K._p, V._p, slopes._p, o._p, hq, hkv, q_len, kv_len, d, float(scale), q_len * d, d, kv_len * d, d,
         q_len * d, d, Q.dtype.code, None)
    return o


def sdpa_alibi_strided(q: GPUArray, k: GPUArray, v: GPUArray, slopes: GPUArray, out: GPUArray, hq: int, hkv: int, q_len: int, kv_len: int,
                       d: int, q_strides, kv_strides, o_strides, scale: float = 0.0) -> None:
    """sdpa_alibi on [S,H,D]-layout (or any head/row-strided) buffers, written into `out`: strides are (head, row) in
    elements, multiples of 8."""
    _check_alibi(q, k, v, out, slopes, hq, hkv, q_len, kv_len, d, "sdpa_alibi_strided")
    if any(int(x) % 8 or int(x) < 0 for x in (*q_strides, *kv_strides, *o_strides)):
        raise ValueError("sdpa_alibi_strided: strides must be non-negative multiples of 8 elements")
    call("pgk_sdpa_alibi", q._p, k._p, v._p, slopes._p, out._p, hq, hkv, q_len, kv_len, d, float(scale), q_strides[0], q_strides[1],
         kv_strides[0], kv_strides[1], o_strides[0], o_strides[1], q.dtype.code, None)


def _check_fixed_cache(Q: GPUArray, K: GPUArray, V: GPUArray, slopes: GPUArray, out: GPUArray, context_len: int, name: str):
    if Q.ndim != 3 or K.ndim != 3 or V.ndim != 3:
        raise ValueError(f"{name} expects 3D Q [Hq, q_len, D] and caches [Hkv, max_seq, D]")
    hq, q_len, d = Q.shape
    hkv, max_seq = K.shape[0], K.shape[1]
    if K.shape != V.shape or K.shape[2] != d or max_seq < 1:
        raise ValueError(f"{name}: caches {K.shape} / {V.shape} do not fit Q {Q.shape}")
    if out.shape != Q.shape:
        raise ValueError(f"{name}: out shape {out.shape} does not match Q {Q.shape}")
    _check_alibi(Q, K, V, out, slopes, hq, hkv, q_len, context_len, d, name)
    return hq, hkv, q_len, max_seq, d


def sdpa_alibi_fixed_cache(Q: GPUArray, K: GPUArray, V: GPUArray, slopes: GPUArray, out: GPUArray, context_len: int,
                           scale: float = 0.0) -> None:
    """sdpa_alibi of Q [Hq, q_len, D] over the first context_len rows of the fixed caches K, V [Hkv, max_seq, D], written
    into `out`: one row is split-KV flash-decoding, more rows run the prefill kernel over the cache in place."""
    hq, hkv, q_len, max_seq, d = _check_fixed_cache(Q, K, V, slopes, out, context_len, "sdpa_alibi_fixed_cache")
    if context_len > max_seq:
        raise ValueError(f"sdpa_alibi_fixed_cache: context_len {context_len} outside cache of {max_seq} rows")
    ws = _workspace(hq, d, max_seq) if q_len == 1 else None
    call("pgk_sdpa_alibi_fixed_cache", Q._p, K._p, V._p, slopes._p, out._p, hq, hkv, q_len, max_seq, d, float(scale), int(context_len), None,
         ws._p if ws is not None else None, Q.dtype.code, None)


def sdpa_alibi_fixed_cache_ptr(Q: GPUArray, K: GPUArray, V: GPUArray, slopes: GPUArray, out: GPUArray, context_len_buf: GPUArray,
                               max_kv_len: int, scale: float = 0.0) -> None:
    """As above for one query row with context_len read from a device int32 (graph replay), clamped to the cache;
    max_kv_len is accepted for symmetry with sdpa_causal_fixed_cache_ptr."""
    name = "sdpa_alibi_fixed_cache_ptr"
    if Q.ndim == 3 and Q.shape[1] != 1:
        raise ValueError(f"{name}: q_len must be 1 with a device context length, got {Q.shape[1]}")
    hq, hkv, q_len, max_seq, d = _check_fixed_cache(Q, K, V, slopes, out, 1, name)
    if context_len_buf.dtype != int32 or context_len_buf.size < 1:
        raise ValueError(f"{name}: context_len_buf must be int32 with at least one element")
    call("pgk_sdpa_alibi_fixed_cache", Q._p, K._p, V._p, slopes._p, out._p, hq, hkv, 1, max_seq, d, float(scale), 0, context_len_buf._p,
         _workspace(hq, d, max_seq)._p, Q.dtype.code, None)


__all__ = ["sdpa_alibi", "sdpa_alibi_strided", "sdpa_alibi_fixed_cache", "sdpa_alibi_fixed_cache_ptr"]
