"""float64 NumPy restatement of sliding-window attention: the mask and the softmax, nothing else.

Query row i of q_len, key j of kv_len, off = kv_len - q_len: key j is visible when max(0, off + i - W + 1) <= j <= off + i."""

from __future__ import annotations

import numpy as np


def window_mask(q_len: int, kv_len: int, window: int) -> np.ndarray:
    """[q_len, kv_len] bool."""
    i, j = np.arange(q_len)[:, None], np.arange(kv_len)[None, :]
    off = kv_len - q_len
    return (j <= off + i) & (j >= off + i - window + 1)


def sdpa_window(q, k, v, window: int, scale: float | None = None) -> np.ndarray:
    """q [Hq, q_len, D], k / v [Hkv, kv_len, D] -> [Hq, q_len, D] in float64; GQA by h // (Hq / Hkv)."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    hq, q_len, d = q.shape
    rep = hq // k.shape[0]
    scale = 1.0 / np.sqrt(d) if scale is None else scale
    seen = window_mask(q_len, k.shape[1], window)
    out = np.empty_like(q)
    for h in range(hq):
        s = np.where(seen, (q[h] @ k[h // rep].T) * scale, -np.inf)
        p = np.exp(s - s.max(axis=1, keepdims=True))
        out[h] = (p / p.sum(axis=1, keepdims=True)) @ v[h // rep]
    return out
