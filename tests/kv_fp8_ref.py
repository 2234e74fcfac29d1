"""NumPy restatement of the FP8 (OCP e4m3) KV cache: the quantiser of the cache writer, its inverse and one-row decode attention.

code = rne_e4m3(clamp(x / scale, +-448)), x widened to float32 and a correctly rounded float32 division; value = table[code] * scale.
scale: one float32 per KV head, broadcast over [.., Hkv, D] (new_kv layout, head_axis=-2) or [Hkv, rows, D] (cache layout, head_axis=0)."""

from __future__ import annotations

import numpy as np

from oracle.cpu_ref import _rne_e4m3_codes, fp8_e4m3_table


def _per_head(scale, ndim: int, head_axis: int) -> np.ndarray:
    shape = [1] * ndim
    shape[head_axis] = -1
    return np.asarray(scale, np.float32).reshape(shape)


def quantise(x, scale, head_axis: int = -2) -> np.ndarray:
    x = np.asarray(x, np.float32)
    return _rne_e4m3_codes((x / _per_head(scale, x.ndim, head_axis)).astype(np.float32))


def dequantise(codes, scale, head_axis: int = 0) -> np.ndarray:
    """float64."""
    codes = np.asarray(codes, np.uint8)
    return fp8_e4m3_table()[codes].astype(np.float64) * _per_head(scale, codes.ndim, head_axis).astype(np.float64)


def absmax_scales(x) -> np.ndarray:
    """float32 [Hkv] of x [S, Hkv, D]: absmax / 224, 1 for an all-zero head."""
    m = np.abs(np.asarray(x, np.float32)).max(axis=(0, 2))
    return np.where(m > 0, m / np.float32(224.0), np.float32(1.0)).astype(np.float32)


def decode(q, k_codes, v_codes, k_scale, v_scale, ctx: int, scale: float | None = None) -> np.ndarray:
    """q [Hq, 1, D], codes [Hkv, rows, D] -> softmax(scale * q K^T) V over rows 0 .. ctx - 1 in float64, [Hq, 1, D]; GQA by h // (Hq / Hkv)."""
    q = np.asarray(q, np.float64)
    k, v = dequantise(k_codes[:, :ctx], k_scale), dequantise(v_codes[:, :ctx], v_scale)
    hq, _, d = q.shape
    rep = hq // k.shape[0]
    scale = 1.0 / np.sqrt(d) if scale is None else scale
    out = np.empty_like(q)
    for h in range(hq):
        s = (q[h] @ k[h // rep].T) * scale
        p = np.exp(s - s.max(axis=1, keepdims=True))
        out[h] = (p / p.sum(axis=1, keepdims=True)) @ v[h // rep]
    return out
