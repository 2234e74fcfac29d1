"""[build-defined] FP8 (OCP e4m3) KV cache: half the bytes a decode step streams, twice the context in the same HBM.

Cache [Hkv, max_seq, D] in uint8 (un-expanded only), one float32 scale per KV head for K and one for V: value = e4m3(code) * scale,
code = rne_e4m3(clamp(x / scale, +-448)) with a correctly rounded float32 division (oracle.cpu_ref._rne_e4m3_codes of x / scale).

  kv_fp8_scales                         per-head absmax / 224 of a [S, Hkv, D] array (1 for an all-zero head)
  kv_cache_update_gqa_fp8 / _ptr        one token's K or V -> cache row `position`
  kv_cache_prefill_gqa_fp8              a prompt's K or V -> rows start_position ..
  sdpa_causal_fixed_cache_fp8 / _ptr    one query row over rows 0 .. context_len - 1 of the dequantised caches (split-KV)
  sdpa_kv_fp8_plan                      ("kv_fp8_split", chunks per kv head); needs no GPU work

bfloat16 / float16 queries, head_dim 64 or 128.  A query of several rows over this contiguous fp8 cache, the window / iRoPE / ALiBi
forms and the native engine have no fp8 kernel; fp8 PAGES are ops.paged's (*_fp8)."""

from __future__ import annotations

import ctypes as C

from pygpukit_amd import _hip
from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import as_dtype, bfloat16, float16, float32, int32, uint8
from pygpukit_amd.ops._common import call
from pygpukit_amd.ops.nn.attention import _workspace


def _check_write(new_kv: GPUArray, cache: GPUArray, scales: GPUArray, name: str):
    if new_kv.ndim != 3 or cache.ndim != 3 or new_kv.dtype not in (bfloat16, float16) or cache.dtype != uint8:
        raise ValueError(f"{name}: new_kv must be bfloat16 / float16 [S, Hkv, D] and cache uint8 [Hkv, max_seq, D], got "
                         f"{new_kv.shape}/{new_kv.dtype} and {cache.shape}/{cache.dtype}")
    s, hkv, d = new_kv.shape
    if cache.shape[0] != hkv or cache.shape[2] != d or d not in (64, 128):
        raise ValueError(f"{name}: new_kv {new_kv.shape} does not fit cache {cache.shape} (un-expanded, head_dim 64 or 128)")
    if scales.dtype != float32 or scales.shape != (hkv,):
        raise ValueError(f"{name}: scales must be float32 [{hkv}], got {scales.shape}/{scales.dtype}")
    return s, hkv, d


def kv_cache_update_gqa_fp8(new_kv: GPUArray, cache: GPUArray, scales: GPUArray, position: int) -> None:
    """new_kv [1, Hkv, D] -> row `position` of the fp8 cache [Hkv, max_seq, D], quantised with scales [Hkv]."""
    kv_cache_prefill_gqa_fp8(new_kv, cache, scales, position)


def kv_cache_update_gqa_fp8_ptr(new_kv: GPUArray, cache: GPUArray, scales: GPUArray, position_buf: GPUArray) -> None:
    """kv_cache_update_gqa_fp8 with the position read from a device int32 (graph replay)."""
    s, hkv, d = _check_write(new_kv, cache, scales, "kv_cache_update_gqa_fp8_ptr")
    if position_buf.dtype != int32:
        raise ValueError("kv_cache_update_gqa_fp8_ptr: position_buf must be int32")
    call("pgk_kv_cache_write_fp8", new_kv._p, cache._p, scales._p, s, hkv, cache.shape[1], d, 0, position_buf._p, new_kv.dtype.code, None)


def kv_cache_prefill_gqa_fp8(new_kv: GPUArray, cache: GPUArray, scales: GPUArray, start_position: int = 0) -> None:
    """new_kv [S, Hkv, D] -> rows start_position .. start_position + S - 1 of the fp8 cache."""
    s, hkv, d = _check_write(new_kv, cache, scales, "kv_cache_prefill_gqa_fp8")
    if start_position < 0 or start_position + s > cache.shape[1]:
        raise ValueError(f"kv_cache_prefill_gqa_fp8: rows {start_position}..{start_position + s - 1} outside cache of {cache.shape[1]}")
    call("pgk_kv_cache_write_fp8", new_kv._p, cache._p, scales._p, s, hkv, cache.shape[1], d, int(start_position), None, new_kv.dtype.code, None)


def kv_fp8_scales(x: GPUArray, num_kv_heads: int, *, out: GPUArray | None = None) -> GPUArray:
    """float32 [Hkv]: max |x[:, h, :]| / 224 of x [S, Hkv, D] - half of the e4m3 range is headroom for later tokens; 1 for a zero head."""
    if x.ndim != 3 or x.shape[1] != num_kv_heads or x.dtype not in (bfloat16, float16) or x.shape[0] < 1 or x.shape[2] % 8:
        raise ValueError(f"kv_fp8_scales: x must be bfloat16 / float16 [S >= 1, {num_kv_heads}, D % 8 == 0], got {x.shape}/{x.dtype}")
    o = out if out is not None else GPUArray((num_kv_heads,), float32)
    if o.dtype != float32 or o.shape != (num_kv_heads,):
        raise ValueError("kv_fp8_scales: out must be float32 [num_kv_heads]")
    call("pgk_kv_fp8_absmax_scales", x._p, o._p, x.shape[0], num_kv_heads, x.shape[2], x.dtype.code, None)
    return o


def _check_decode(q, k_cache, v_cache, k_scale, v_scale, out, name):
    if q.ndim != 3 or q.shape[1] != 1 or q.dtype not in (bfloat16, float16):
        raise ValueError(f"{name}: q must be bfloat16 / float16 [Hq, 1, D] (a query of several rows has no fp8-cache kernel), got "
                         f"{q.shape}/{q.dtype}")
    hq, _, d = q.shape
    if k_cache.ndim != 3 or k_cache.dtype != uint8 or v_cache.dtype != uint8 or k_cache.shape != v_cache.shape or k_cache.shape[2] != d:
        raise ValueError(f"{name}: caches must be uint8 [Hkv, max_seq, {d}], got {k_cache.shape}/{k_cache.dtype} and {v_cache.shape}/{v_cache.dtype}")
    hkv, max_seq = k_cache.shape[0], k_cache.shape[1]
    if hq % hkv or d not in (64, 128):
        raise ValueError(f"{name}: needs Hq % Hkv == 0 and head_dim 64 or 128 (got heads {hq}/{hkv}, D {d})")
    for sc in (k_scale, v_scale):
        if sc.dtype != float32 or sc.shape != (hkv,):
            raise ValueError(f"{name}: k_scale / v_scale must be float32 [{hkv}]")
    if out.shape != q.shape or out.dtype != q.dtype:
        raise ValueError(f"{name}: output shape/dtype mismatch")
    return hq, hkv, max_seq, d


def sdpa_causal_fixed_cache_fp8(q: GPUArray, k_cache: GPUArray, v_cache: GPUArray, k_scale: GPUArray, v_scale: GPUArray, out: GPUArray,
                                context_len: int, scale: float = 0.0) -> None:
    """softmax(scale * q K^T) V of q [Hq, 1, D] over rows 0 .. context_len - 1 of the fp8 caches; scale <= 0 -> 1/sqrt(D).  Rows at
    and beyond context_len are never read."""
    hq, hkv, max_seq, d = _check_decode(q, k_cache, v_cache, k_scale, v_scale, out, "sdpa_causal_fixed_cache_fp8")
    if context_len <= 0 or context_len > max_seq:
        raise ValueError(f"sdpa_causal_fixed_cache_fp8: invalid context_len {context_len}")
    call("pgk_sdpa_fixed_cache_fp8", q._p, k_cache._p, v_cache._p, k_scale._p, v_scale._p, out._p, hq, hkv, max_seq, d, float(scale),
         int(context_len), None, _workspace(hq, d, max_seq)._p, q.dtype.code, None)


def sdpa_causal_fixed_cache_fp8_ptr(q: GPUArray, k_cache: GPUArray, v_cache: GPUArray, k_scale: GPUArray, v_scale: GPUArray, out: GPUArray,
                                    context_len_buf: GPUArray, max_kv_len: int = 0, scale: float = 0.0) -> None:
    """As above with context_len read from a device int32 (graph replay) and clamped to the cache; the grid depends on max_seq only
    (max_kv_len is accepted for the signature of sdpa_causal_fixed_cache_ptr and not used)."""
    hq, hkv, max_seq, d = _check_decode(q, k_cache, v_cache, k_scale, v_scale, out, "sdpa_causal_fixed_cache_fp8_ptr")
    if context_len_buf.dtype != int32:
        raise ValueError("sdpa_causal_fixed_cache_fp8_ptr: context_len_buf must be int32")
    call("pgk_sdpa_fixed_cache_fp8", q._p, k_cache._p, v_cache._p, k_scale._p, v_scale._p, out._p, hq, hkv, max_seq, d, float(scale), 0,
         context_len_buf._p, _workspace(hq, d, max_seq)._p, q.dtype.code, None)


def sdpa_kv_fp8_plan(hq: int, hkv: int, head_dim: int, max_seq: int, dtype, aligned: bool = True) -> tuple[str, int]:
    """("kv_fp8_split", chunks per kv head) of sdpa_causal_fixed_cache_fp8 for this shape; ValueError for what the op rejects."""
    lib = _hip.load()
    nsplit = C.c_int(0)
    plan = lib.pgk_sdpa_kv_fp8_plan(int(hq), int(hkv), int(head_dim), int(max_seq), as_dtype(dtype).code, int(bool(aligned)), C.byref(nsplit))
    if plan is None:
        msg = lib.pgk_last_error()
        raise ValueError(msg.decode(errors="replace") if msg else "sdpa_kv_fp8_plan: invalid call")
    return plan.decode(), nsplit.value


__all__ = ["kv_cache_update_gqa_fp8", "kv_cache_update_gqa_fp8_ptr", "kv_cache_prefill_gqa_fp8", "kv_fp8_scales", "sdpa_causal_fixed_cache_fp8",
           "sdpa_causal_fixed_cache_fp8_ptr", "sdpa_kv_fp8_plan"]
