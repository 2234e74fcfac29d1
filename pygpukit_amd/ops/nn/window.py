"""[build-defined] Sliding-window attention (Mistral, Phi-3, Gemma's local layers, Qwen2's use_sliding_window).

Query row i of q_len sees the keys max(0, off + i - window + 1) .. off + i with off = kv_len - q_len: `window` keys including its
own (HuggingFace's kv_idx > q_idx - sliding_window).  window >= kv_len is plain causal attention.

  sdpa_sliding_window / _strided        prefill: the flash kernel's FlashWindow policy - a query tile walks only the KV tiles of its band
  sdpa_sliding_window_fixed_cache/_ptr  one query row over a fixed cache; the split-KV chunks cut the window, not the cache
  kv_cache_update_ring / _ptr           the writer of a rolling cache [Hc, C, D]: position p lives in row p % C
  sdpa_window_plan                      (kernel, KV runs per query tile) of a prefill call; needs no GPU work
"""

from __future__ import annotations

import ctypes as C

from pygpukit_amd import _hip
from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import as_dtype, int32
from pygpukit_amd.ops._common import call, check_out
from pygpukit_amd.ops.nn.attention import _check_qkv, _workspace


def _check_window(window, name: str) -> int:
    if isinstance(window, bool) or int(window) != window or window < 1:
        raise ValueError(f"{name}: window must be an integer >= 1, got {window!r}")
    return min(int(window), 2 ** 31 - 1)


def sdpa_sliding_window(Q: GPUArray, K: GPUArray, V: GPUArray, window: int, scale: float = 0.0, *, out: GPUArray | None = None) -> GPUArray:
    """softmax(Q K^T * scale + band mask) V: Q [Hq, q_len, D], K / V [Hkv, kv_len, D], kv_len >= q_len >= 1, window >= 1;
    scale <= 0 -> 1/sqrt(head_dim).  bfloat16 / float16 with head_dim 64 or 128 run the MFMA flash kernel at every q_len;
    float32, other head dims and PYGPUKIT_FLASH_ATTENTION=0 the fallback."""
    hq, hkv, q_len, kv_len, d = _check_qkv(Q, K, V, "sdpa_sliding_window")
    w = _check_window(window, "sdpa_sliding_window")
    if q_len < 1 or kv_len < q_len:
        raise ValueError(f"sdpa_sliding_window: needs kv_len >= q_len >= 1, got q_len {q_len}, kv_len {kv_len}")
    o = check_out(out, (hq, q_len, d), Q.dtype, "sdpa_sliding_window")
    call("pgk_sdpa_window", Q._p, K._p, V._p, o._p, hq, hkv, q_len, kv_len, d, w, float(scale), q_len * d, d, kv_len * d, d, q_len * d, d,
         Q.dtype.code, None)
    return o


def sdpa_sliding_window_strided(q: GPUArray, k: GPUArray, v: GPUArray, out: GPUArray, hq: int, hkv: int, q_len: int, kv_len: int, d: int,
                                window: int, q_strides, kv_strides, o_strides, scale: float = 0.0) -> None:
    """sdpa_sliding_window on [S,H,D]-layout (or any head/row-strided) buffers: strides are (head, row) in elements."""
    w = _check_window(window, "sdpa_sliding_window_strided")
    if hq < 1 or hkv < 1 or hq % hkv:
        raise ValueError("sdpa_sliding_window_strided: n_heads mismatch")
    if q_len < 1 or kv_len < q_len or d < 1:
        raise ValueError(f"sdpa_sliding_window_strided: needs kv_len >= q_len >= 1 and head_dim >= 1, got {q_len}, {kv_len}, {d}")
    if any(int(x) < 0 for x in (*q_strides, *kv_strides, *o_strides)):
        raise ValueError("sdpa_sliding_window_strided: strides must be non-negative")
    call("pgk_sdpa_window", q._p, k._p, v._p, out._p, hq, hkv, q_len, kv_len, d, w, float(scale), q_strides[0], q_strides[1], kv_strides[0],
         kv_strides[1], o_strides[0], o_strides[1], q.dtype.code, None)


def _check_fixed(Q, K, V, out, window, name):
    hq, hc, q_len, rows, d = _check_qkv(Q, K, V, name)
    w = _check_window(window, name)
    if q_len != 1:
        raise ValueError(f"{name}: q_len must be 1 (a chunk over a linear cache is sdpa_sliding_window_strided on the cache prefix)")
    if out.shape != (hq, 1, d) or out.dtype != Q.dtype:
        raise ValueError(f"{name}: output shape/dtype mismatch")
    return hq, hc, rows, d, w


def sdpa_sliding_window_fixed_cache(Q: GPUArray, K: GPUArray, V: GPUArray, out: GPUArray, context_len: int, window: int, scale: float = 0.0,
                                    *, ring: bool = False) -> None:
    """Q [Hq, 1, D] over positions max(0, context_len - window) .. context_len - 1 of the caches K, V [Hc, rows, D].  ring=False:
    position p is row p and context_len <= rows.  ring=True: position p is row p % rows (kv_cache_update_ring) and context_len
    may pass rows when window <= rows."""
    hq, hc, rows, d, w = _check_fixed(Q, K, V, out, window, "sdpa_sliding_window_fixed_cache")
    if context_len <= 0 or (context_len > rows and not (ring and w <= rows)):
        raise ValueError(f"sdpa_sliding_window_fixed_cache: invalid context_len {context_len} (cache rows {rows}, window {w}, ring {ring})")
    ws = _workspace(hq, d, min(rows, w)) if d in (64, 128) else None
    call("pgk_sdpa_window_fixed_cache", Q._p, K._p, V._p, out._p, hq, hc, rows, d, w, int(bool(ring)), float(scale), int(context_len), None,
         ws._p if ws is not None else None, Q.dtype.code, None)


def sdpa_sliding_window_fixed_cache_ptr(Q: GPUArray, K: GPUArray, V: GPUArray, out: GPUArray, context_len_buf: GPUArray, window: int,
                                        scale: float = 0.0, *, ring: bool = False) -> None:
    """As above with context_len read from a device int32 (graph replay): the grid depends on min(rows, window) only."""
    hq, hc, rows, d, w = _check_fixed(Q, K, V, out, window, "sdpa_sliding_window_fixed_cache_ptr")
    if context_len_buf.dtype != int32:
        raise ValueError("sdpa_sliding_window_fixed_cache_ptr: context_len_buf must be int32")
    if d not in (64, 128):
        raise ValueError(f"sdpa_sliding_window_fixed_cache_ptr: head_dim must be 64 or 128, got {d}")
    if ring and w > rows:
        raise ValueError(f"sdpa_sliding_window_fixed_cache_ptr: a ring of {rows} rows cannot hold a window of {w}")
    ws = _workspace(hq, d, min(rows, w))
    call("pgk_sdpa_window_fixed_cache", Q._p, K._p, V._p, out._p, hq, hc, rows, d, w, int(bool(ring)), float(scale), 0, context_len_buf._p,
         ws._p, Q.dtype.code, None)


def _check_ring(new_kv: GPUArray, cache: GPUArray, num_heads: int, name: str):
    if new_kv.ndim != 3 or cache.ndim != 3 or new_kv.dtype != cache.dtype or new_kv.shape[2] != cache.shape[2]:
        raise ValueError(f"{name}: new_kv {new_kv.shape}/{new_kv.dtype} does not fit cache {cache.shape}/{cache.dtype}")
    hkv, hc = new_kv.shape[1], cache.shape[0]
    if hc not in (hkv, num_heads) or hc % hkv:
        raise ValueError(f"{name}: cache heads {hc} must be num_kv_heads {hkv} or num_heads {num_heads}")
    if new_kv.shape[0] > cache.shape[1]:
        raise ValueError(f"{name}: {new_kv.shape[0]} rows do not fit a ring of {cache.shape[1]}")
    return hkv, hc


def kv_cache_update_ring(new_kv: GPUArray, cache: GPUArray, num_heads: int, position: int) -> None:
    """new_kv [S, Hkv, D] (S <= C) -> rows (position + s) % C of the rolling cache [Hc, C, D]."""
    hkv, hc = _check_ring(new_kv, cache, num_heads, "kv_cache_update_ring")
    if position < 0:
        raise ValueError(f"kv_cache_update_ring: negative position {position}")
    call("pgk_kv_cache_write_ring", new_kv._p, cache._p, new_kv.shape[0], hkv, hc, cache.shape[1], cache.shape[2], cache.itemsize,
         int(position), None, None)


def kv_cache_update_ring_ptr(new_kv: GPUArray, cache: GPUArray, num_heads: int, position_buf: GPUArray) -> None:
    """kv_cache_update_ring with the position read from a device int32 (graph replay)."""
    hkv, hc = _check_ring(new_kv, cache, num_heads, "kv_cache_update_ring_ptr")
    if position_buf.dtype != int32:
        raise ValueError("kv_cache_update_ring_ptr: position_buf must be int32")
    call("pgk_kv_cache_write_ring", new_kv._p, cache._p, new_kv.shape[0], hkv, hc, cache.shape[1], cache.shape[2], cache.itemsize, 0,
         position_buf._p, None)


def sdpa_window_plan(hq: int, hkv: int, q_len: int, kv_len: int, head_dim: int, window: int, dtype, aligned: bool = True) -> tuple[str, int]:
    """("window_flash" | "window_rows", KV runs per query tile) of sdpa_sliding_window for this shape on the current device."""
    lib = _hip.load()
    nsplit = C.c_int(0)
    plan = lib.pgk_sdpa_window_plan(int(hq), int(hkv), int(q_len), int(kv_len), int(head_dim), min(int(window), 2 ** 31 - 1),
                                    as_dtype(dtype).code, int(bool(aligned)), C.byref(nsplit))
    if plan is None:
        msg = lib.pgk_last_error()
        raise ValueError(msg.decode(errors="replace") if msg else "sdpa_window_plan: invalid call")
    return plan.decode(), nsplit.value


__all__ = ["sdpa_sliding_window", "sdpa_sliding_window_strided", "sdpa_sliding_window_fixed_cache", "sdpa_sliding_window_fixed_cache_ptr",
           "kv_cache_update_ring", "kv_cache_update_ring_ptr", "sdpa_window_plan"]
