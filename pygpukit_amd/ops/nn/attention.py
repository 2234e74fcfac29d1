"""Causal scaled-dot-product attention (reference: src/pygpukit/ops/nn/attention.py:16-235 ->
ops.cuh:287-300).  K/V may carry fewer heads than Q (un-expanded GQA): kv head = q head // (Hq/Hkv).
sdpa_causal_fp8 (reference :238-347) is the same op with Q.K^T on fp8 codes; its contract is in INTEGRATION.md."""

from __future__ import annotations

import ctypes as C

from pygpukit_amd import _hip
from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import bfloat16, float32, int32, uint8
from pygpukit_amd.ops._common import call, check_out, validate_float

_ws_cache: dict[tuple[int, int, int], GPUArray] = {}


def _check_qkv(Q: GPUArray, K: GPUArray, V: GPUArray, name: str):
    validate_float(Q, name)
    if Q.ndim != 3 or K.ndim != 3 or V.ndim != 3:
        raise ValueError(f"{name} expects 3D inputs [n_heads, seq_len, head_dim]")
    if Q.dtype != K.dtype or Q.dtype != V.dtype:
        raise ValueError(f"{name}: Q, K, V must have same dtype")
    hq, q_len, d = Q.shape
    if K.shape[0] != V.shape[0] or hq % K.shape[0] != 0:
        raise ValueError(f"{name}: n_heads mismatch")
    if K.shape[2] != d or V.shape[2] != d:
        raise ValueError(f"{name}: head_dim mismatch")
    if K.shape[1] != V.shape[1]:
        raise ValueError(f"{name}: K and V seq_len mismatch")
    return hq, K.shape[0], q_len, K.shape[1], d


def sdpa_causal(Q: GPUArray, K: GPUArray, V: GPUArray, scale: float = 0.0, *, out: GPUArray | None = None) -> GPUArray:
    """softmax(Q K^T * scale + causal mask) V; scale <= 0 -> 1/sqrt(head_dim); the mask lets query i see
    kv positions <= (kv_len - q_len) + i."""
    hq, hkv, q_len, kv_len, d = _check_qkv(Q, K, V, "sdpa_causal")
    o = check_out(out, (hq, q_len, d), Q.dtype, "sdpa_causal")
    call("pgk_sdpa_causal", Q._p, K._p, V._p, o._p, hq, hkv, q_len, kv_len, d, float(scale), q_len * d, d, kv_len * d, d,
         q_len * d, d, Q.dtype.code, None)
    return o


def sdpa_causal_strided(q: GPUArray, k: GPUArray, v: GPUArray, out: GPUArray, hq: int, hkv: int, q_len: int, kv_len: int,
                        d: int, q_strides, kv_strides, o_strides, scale: float = 0.0) -> None:
    """Same op on [S,H,D]-layout (or any head/row-strided) buffers: strides are (head, row) in elements."""
    call("pgk_sdpa_causal", q._p, k._p, v._p, out._p, hq, hkv, q_len, kv_len, d, float(scale), q_strides[0], q_strides[1],
         kv_strides[0], kv_strides[1], o_strides[0], o_strides[1], q.dtype.code, None)


def sdpa_noncausal(Q: GPUArray, K: GPUArray, V: GPUArray, scale: float = 0.0, *, out: GPUArray | None = None) -> GPUArray:
    """[build-defined] softmax(Q K^T * scale) V with every key visible to every query: Q [Hq, q_len, D], K / V [Hkv, kv_len, D],
    any q_len and kv_len >= 1 (encoders, cross-attention); scale <= 0 -> 1/sqrt(head_dim).  bfloat16 / float16 with head_dim 64 or
    128 run the MFMA flash kernel at every q_len; float32, other head dims and PYGPUKIT_FLASH_ATTENTION=0 the fallback."""
    hq, hkv, q_len, kv_len, d = _check_qkv(Q, K, V, "sdpa_noncausal")
    if min(q_len, kv_len, d) < 1:
        raise ValueError(f"sdpa_noncausal: empty dimension, Q {Q.shape} K {K.shape}")
    o = check_out(out, (hq, q_len, d), Q.dtype, "sdpa_noncausal")
    call("pgk_sdpa_noncausal", Q._p, K._p, V._p, o._p, hq, hkv, q_len, kv_len, d, float(scale), q_len * d, d, kv_len * d, d,
         q_len * d, d, Q.dtype.code, None)
    return o


def sdpa_noncausal_strided(q: GPUArray, k: GPUArray, v: GPUArray, out: GPUArray, hq: int, hkv: int, q_len: int, kv_len: int,
                           d: int, q_strides, kv_strides, o_strides, scale: float = 0.0) -> None:
    """sdpa_noncausal on [S,H,D]-layout (or any head/row-strided) buffers: strides are (head, row) in elements, so the
    [S, 3*H*D] output of a fused QKV projection is read in place."""
    if hq < 1 or hkv < 1 or hq % hkv:
        raise ValueError("sdpa_noncausal_strided: n_heads mismatch")
    if min(q_len, kv_len, d) < 1:
        raise ValueError(f"sdpa_noncausal_strided: needs q_len, kv_len, head_dim >= 1, got {q_len}, {kv_len}, {d}")
    if any(int(x) < 0 for x in (*q_strides, *kv_strides, *o_strides)):
        raise ValueError("sdpa_noncausal_strided: strides must be non-negative")
    call("pgk_sdpa_noncausal", q._p, k._p, v._p, out._p, hq, hkv, q_len, kv_len, d, float(scale), q_strides[0], q_strides[1],
         kv_strides[0], kv_strides[1], o_strides[0], o_strides[1], q.dtype.code, None)


def get_sm_version() -> int:
    """The reference returns the CUDA SM version (120 for SM120).  Here the number is the gfx target of the current
    device - the decimal digits after "gfx" in its architecture name: 950 on MI355X (gfx950)."""
    gfx = C.c_int(0)
    call("pgk_device_arch", C.byref(gfx))
    return gfx.value


def fa3_fp8_available() -> bool:
    """True when sdpa_causal_fp8 can run: the current device is gfx950 (the fp8 MFMA the kernel is written for).
    False on any other device, and False - not an error - when there is no device or no library."""
    try:
        return _hip.device_count() > 0 and get_sm_version() == 950
    except RuntimeError:
        return False


def _check_fp8(q: GPUArray, k: GPUArray, v: GPUArray, out: GPUArray, d: int) -> None:
    if not fa3_fp8_available():
        raise RuntimeError("FA3 FP8 requires a gfx950 device (MI355X)")
    validate_float(q, "sdpa_causal_fp8")
    if q.dtype != k.dtype or q.dtype != v.dtype or q.dtype != bfloat16:
        raise ValueError("sdpa_causal_fp8: Q, K, V must have same dtype (BFloat16)")
    if out.dtype != q.dtype:
        raise ValueError("sdpa_causal_fp8: out must have same dtype as Q")
    if d != 128:
        raise ValueError(f"sdpa_causal_fp8: head_dim must be 128, got {d}")


def _check_fp8_shape(hq: int, hkv: int, q_len: int, kv_len: int) -> None:
    if hq <= 0 or hkv <= 0 or hq % hkv != 0:
        raise ValueError("sdpa_causal_fp8: n_heads mismatch")
    if q_len < 1 or kv_len < q_len:
        raise ValueError(f"sdpa_causal_fp8: needs kv_len >= q_len >= 1, got q_len {q_len}, kv_len {kv_len}")


def sdpa_causal_fp8(Q: GPUArray, K: GPUArray, V: GPUArray, out: GPUArray, scale: float = 0.0) -> None:
    """sdpa_causal with the first product in fp8: Q (per query head) and K (per kv head) are quantised to e4m3 with one
    power-of-two scale per head, Q.K^T runs on the fp8 MFMA with fp32 sums, softmax is fp32, P.V uses V unquantised in
    bf16.  BFloat16 only, head_dim 128; writes `out` [Hq, q_len, 128] in place.  scale <= 0 -> 1/sqrt(head_dim).
    K/V may carry fewer heads than Q (un-expanded GQA), as in sdpa_causal."""
    if Q.ndim != 3 or K.ndim != 3 or V.ndim != 3:
        raise ValueError("sdpa_causal_fp8 expects 3D inputs [n_heads, seq_len, head_dim]")
    _check_fp8(Q, K, V, out, Q.shape[2])
    hq, q_len, d = Q.shape
    if K.shape[0] != V.shape[0] or hq % K.shape[0] != 0:
        raise ValueError("sdpa_causal_fp8: n_heads mismatch")
    if K.shape[2] != d or V.shape[2] != d:
        raise ValueError("sdpa_causal_fp8: head_dim mismatch")
    if K.shape[1] != V.shape[1]:
        raise ValueError("sdpa_causal_fp8: K and V seq_len mismatch")
    if out.shape != (hq, q_len, d):
        raise ValueError(f"out shape {out.shape} does not match expected {(hq, q_len, d)}")
    kv_len = K.shape[1]
    _check_fp8_shape(hq, K.shape[0], q_len, kv_len)
    call("pgk_sdpa_causal_fp8", Q._p, K._p, V._p, out._p, hq, K.shape[0], q_len, kv_len, d, float(scale), q_len * d, d, kv_len * d, d,
         q_len * d, d, Q.dtype.code, None)


def sdpa_causal_fp8_strided(q: GPUArray, k: GPUArray, v: GPUArray, out: GPUArray, hq: int, hkv: int, q_len: int, kv_len: int,
                            d: int, q_strides, kv_strides, o_strides, scale: float = 0.0) -> None:
    """sdpa_causal_fp8 on [S,H,D]-layout (or any head/row-strided) buffers: strides are (head, row) in elements."""
    _check_fp8(q, k, v, out, d)
    _check_fp8_shape(hq, hkv, q_len, kv_len)
    if any(int(x) % 8 for x in (*q_strides, *kv_strides, *o_strides)):
        raise ValueError("sdpa_causal_fp8_strided: strides must be multiples of 8 elements")
    call("pgk_sdpa_causal_fp8", q._p, k._p, v._p, out._p, hq, hkv, q_len, kv_len, d, float(scale), q_strides[0], q_strides[1],
         kv_strides[0], kv_strides[1], o_strides[0], o_strides[1], q.dtype.code, None)


def quantize_fp8_per_head(x: GPUArray, strides=None, shape=None) -> tuple[GPUArray, GPUArray]:
    """[build-defined] The quantiser sdpa_causal_fp8 applies to Q and K, on its own: x bf16 [H, rows, 128] ->
    (codes uint8 [H, rows, 128], scale_bytes uint8 [H]).  Per head: e = 0 for an all-zero head, else the smallest
    integer with 448 * 2^e >= max|x| (clamped to [-127, 127]); scale byte = e + 127 (UE8M0); code = e4m3(x * 2^-e),
    round-to-nearest-even.  `strides` = (head, row) in elements with `shape` = (H, rows, 128) reads another layout
    (e.g. [S,H,D]) out of the same buffer."""
    if x.dtype != bfloat16:
        raise ValueError("quantize_fp8_per_head: x must be BFloat16")
    h, rows, d = tuple(shape) if shape is not None else x.shape
    if d != 128:
        raise ValueError(f"quantize_fp8_per_head: head_dim must be 128, got {d}")
    sh, ss = strides if strides is not None else (rows * d, d)
    codes, sb = GPUArray((h, rows, d), uint8), GPUArray((h,), uint8)
    call("pgk_quantize_fp8_per_head", x._p, codes._p, sb._p, h, rows, d, sh, ss, x.dtype.code, None)
    return codes, sb


def _workspace(hq: int, d: int, max_seq: int) -> GPUArray:
    key = (hq, d, max_seq)
    ws = _ws_cache.get(key)
    if ws is None:
        nbytes = _hip.load().pgk_sdpa_decode_workspace_bytes(hq, d, max_seq)
        ws = GPUArray(((nbytes + 3) // 4,), float32)
        _ws_cache[key] = ws
    return ws


def sdpa_causal_fixed_cache(Q: GPUArray, K: GPUArray, V: GPUArray, out: GPUArray, context_len: int, scale: float = 0.0) -> None:
    """Attention of Q [Hq,q_len,D] over the first context_len rows of the fixed caches K,V [Hc,max_seq,D]."""
    hq, hc, q_len, max_seq, d = _check_qkv(Q, K, V, "sdpa_causal_fixed_cache")
    if out.shape != (hq, q_len, d) or out.dtype != Q.dtype:
        raise ValueError("sdpa_causal_fixed_cache: output shape/dtype mismatch")
    if context_len <= 0 or context_len > max_seq:
        raise ValueError(f"sdpa_causal_fixed_cache: invalid context_len {context_len}")
    ws = _workspace(hq, d, max_seq) if q_len == 1 else None
    call("pgk_sdpa_fixed_cache", Q._p, K._p, V._p, out._p, hq, hc, q_len, max_seq, d, float(scale), context_len, None,
         ws._p if ws is not None else None, Q.dtype.code, None)


def sdpa_causal_fixed_cache_ptr(Q: GPUArray, K: GPUArray, V: GPUArray, out: GPUArray, context_len_buf: GPUArray,
                                max_kv_len: int, scale: float = 0.0) -> None:
    """As above with context_len read from a device int32 (graph replay)."""
    hq, hc, q_len, max_seq, d = _check_qkv(Q, K, V, "sdpa_causal_fixed_cache_ptr")
    if context_len_buf.dtype != int32:
        raise ValueError("sdpa_causal_fixed_cache_ptr: context_len_buf must be int32")
    if q_len != 1:
        raise ValueError("sdpa_causal_fixed_cache_ptr: q_len must be 1")
    ws = _workspace(hq, d, max_seq)
    call("pgk_sdpa_fixed_cache", Q._p, K._p, V._p, out._p, hq, hc, q_len, max_seq, d, float(scale), 0, context_len_buf._p,
         ws._p, Q.dtype.code, None)
