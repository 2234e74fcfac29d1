"""NumPy restatement of the positional-encoding ops (reference: src/pygpukit/ops/nn/rope.py:136-653, its CPU path) and of
sdpa_alibi.  The tables, slopes, bias and in-place ops are written so that every rounding is explicit (float32 after each
step): they agree bit for bit with what the reference's CPU path returns (tests/golden/g8_posenc.npz) whatever NumPy's
scalar promotion rules are.  sdpa_alibi is an fp64 softmax over the formula of INTEGRATION.md, GQA-aware."""

from __future__ import annotations

import math

import numpy as np

F32 = np.float32


def _inv_freq(head_dim: int, base: float) -> np.ndarray:
    half = head_dim // 2
    expo = np.arange(half, dtype=F32) / F32(half)
    return (F32(1.0) / np.power(F32(base), expo, dtype=F32)).astype(F32)


def _tables(positions: np.ndarray, inv_freq: np.ndarray, layout: str):
    angles = (positions.astype(F32)[:, None] * inv_freq.astype(F32)[None, :]).astype(F32)
    c, s = np.cos(angles), np.sin(angles)
    assert c.dtype == F32
    if layout == "half":
        return np.concatenate([c, c], axis=-1), np.concatenate([s, s], axis=-1)
    assert layout == "interleaved"
    ci, si = np.empty((c.shape[0], 2 * c.shape[1]), F32), np.empty((c.shape[0], 2 * c.shape[1]), F32)
    ci[:, 0::2], ci[:, 1::2], si[:, 0::2], si[:, 1::2] = c, c, s, s
    return ci, si


def rope_init_ntk_aware(max_seq_len, head_dim, base=10000.0, scale=1.0, layout="interleaved"):
    b = base * (scale ** (head_dim / (head_dim - 2))) if scale > 1.0 else base       # Python floats, then one cast
    return _tables(np.arange(max_seq_len, dtype=F32), _inv_freq(head_dim, b), layout)


def rope_init_linear(max_seq_len, head_dim, base=10000.0, scale=1.0, layout="interleaved"):
    return _tables(np.arange(max_seq_len, dtype=F32) / F32(scale), _inv_freq(head_dim, base), layout)


def yarn_inv_freq(head_dim, base, scale, original_max_len, beta_fast, beta_slow):
    """(interpolated inverse frequencies, the ramp): ramp 0 = divided by `scale`, 1 = untouched."""
    inv = _inv_freq(head_dim, base)
    wavelengths = (F32(2 * np.pi) / inv).astype(F32)
    low, high = original_max_len / beta_slow, original_max_len / beta_fast
    smooth = np.clip(((wavelengths - F32(high)) / F32(low - high)).astype(F32), F32(0), F32(1))
    scaled = (inv / F32(scale)).astype(F32)
    return (((F32(1) - smooth) * scaled).astype(F32) + (smooth * inv).astype(F32)).astype(F32), smooth


def rope_init_yarn(max_seq_len, head_dim, base=10000.0, scale=1.0, original_max_len=4096, beta_fast=32.0, beta_slow=1.0, mscale=0.1,
                   layout="interleaved"):
    inv, _ = yarn_inv_freq(head_dim, base, scale, original_max_len, beta_fast, beta_slow)
    c, s = _tables(np.arange(max_seq_len, dtype=F32), inv, layout)
    if mscale > 0:
        f = yarn_mscale_factor(scale, mscale)
        c, s = (c * f).astype(F32), (s * f).astype(F32)
    return c, s


def yarn_mscale_factor(scale, mscale) -> np.float32:
    return F32(mscale * math.log(scale) + 1.0)


def pope_init_encoding(max_seq_len, head_dim, base=10000.0):
    s, c = _tables(np.arange(max_seq_len, dtype=F32), _inv_freq(head_dim, base), "half")[::-1]
    half = head_dim // 2
    enc = np.empty((max_seq_len, head_dim), F32)
    enc[:, 0::2], enc[:, 1::2] = s[:, :half], c[:, :half]
    return enc


def round_to(x32: np.ndarray, dtype: str) -> np.ndarray:
    """float32 values -> the nearest value of `dtype` ("f32", "f16", "bf16"; ties to even), as float32."""
    x32 = np.ascontiguousarray(x32, F32)
    if dtype == "f32":
        return x32
    if dtype == "f16":
        return x32.astype(np.float16).astype(F32)
    u = x32.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16).astype(np.uint32)
    return u.view(F32)


def pope_inplace(q, k, encoding, start_pos=0, dtype="f32"):
    """q [S, Hq, D], k [S, Hk, D] as float32 values of `dtype` -> (q', k'): one fp32 add, one rounding."""
    S = q.shape[0]
    e = encoding[start_pos:start_pos + S].astype(F32)[:, None, :]
    return round_to(q.astype(F32) + e, dtype), round_to(k.astype(F32) + e, dtype)


def alibi_init_slopes(num_heads):
    return np.array([F32(2 ** (-8 * (h + 1) / num_heads)) for h in range(num_heads)], F32)


def alibi_compute_bias(seq_len, num_heads, slopes, causal=True):
    i = np.arange(seq_len)
    dist = (i[:, None] - i[None, :]).astype(F32)
    bias = ((-slopes.astype(F32))[:, None, None] * dist[None]).astype(F32)
    if causal:
        bias[:, i[None, :] > i[:, None]] = F32(-1e9)
    return bias


def alibi_add_bias(scores, slopes, start_pos=0):
    """scores [B, H, q_len, kv_len] fp32 -> a new array: the product and the difference are each rounded to fp32."""
    _, _, q_len, kv_len = scores.shape
    dist = (start_pos + np.arange(q_len)[:, None] - np.arange(kv_len)[None, :]).astype(F32)
    prod = (slopes.astype(F32)[None, :, None, None] * dist[None, None]).astype(F32)
    return (scores.astype(F32) - prod).astype(F32)


def sdpa_alibi(q, k, v, slopes, scale=0.0):
    """q [Hq, q_len, D], k / v [Hkv, kv_len, D], slopes [Hq] -> fp64 [Hq, q_len, D]:
    softmax_j(q.k * scale - slope * (off + i - j), j <= off + i) . v with off = kv_len - q_len."""
    hq, q_len, d = q.shape
    hkv, kv_len = k.shape[0], k.shape[1]
    rep, off = hq // hkv, kv_len - q_len
    if scale <= 0:
        scale = 1.0 / math.sqrt(d)
    i, j = np.arange(q_len)[:, None], np.arange(kv_len)[None, :]
    dist, seen = (off + i - j).astype(np.float64), j <= off + i
    out = np.empty((hq, q_len, d), np.float64)
    for h in range(hq):
        s = q[h].astype(np.float64) @ k[h // rep].astype(np.float64).T * scale - float(slopes[h]) * dist
        s = np.where(seen, s, -np.inf)
        p = np.exp(s - s.max(axis=1, keepdims=True))
        out[h] = (p / p.sum(axis=1, keepdims=True)) @ v[h // rep].astype(np.float64)
    return out


def sdpa_with_bias(q, k, v, bias, scale=0.0):
    """Attention over materialised scores: softmax(q.k * scale + bias[h]) . v, q_len == kv_len, fp64."""
    hq, _, d = q.shape
    rep = hq // k.shape[0]
    if scale <= 0:
        scale = 1.0 / math.sqrt(d)
    out = np.empty(q.shape, np.float64)
    for h in range(hq):
        s = q[h].astype(np.float64) @ k[h // rep].astype(np.float64).T * scale + bias[h].astype(np.float64)
        p = np.exp(s - s.max(axis=1, keepdims=True))
        out[h] = (p / p.sum(axis=1, keepdims=True)) @ v[h // rep].astype(np.float64)
    return out
