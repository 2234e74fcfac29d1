"""Rotary position embedding, in place (reference: src/pygpukit/ops/nn/rope.py:16-133 -> ops.cuh:218-224).
q [S,Hq,D], k [S,Hk,D], cos/sin [S,D]; rotate-half, only table columns d < D/2 are read.

And the positional-encoding family of the same reference file (:136-653): RoPE scaling tables (NTK-aware, YaRN, linear),
the additive sinusoidal encoding PoPE, and ALiBi slopes / bias.  The tables are one-time and tiny: they are computed on the
host with the reference's CPU-path arithmetic (`*_host` functions, NumPy in, NumPy out) and uploaded, so they are bit-identical
to what that path returns; pope_inplace, alibi_compute_bias and alibi_add_bias are kernels (csrc/ops_posenc.hip).  ALiBi
inside attention is ops/nn/alibi.py.  Contract, and where the reference's CPU and device paths disagree: INTEGRATION.md."""

from __future__ import annotations

import math

import numpy as np

from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import float32
from pygpukit_amd.core.factory import from_numpy
from pygpukit_amd.ops._common import call, validate_float


def _rope(q: GPUArray, k: GPUArray, cos: GPUArray, sin: GPUArray, f32_table: bool, name: str) -> None:
    validate_float(q, name)
    if q.ndim != 3 or k.ndim != 3:
        raise ValueError(f"{name} expects 3D q, k [seq_len, n_heads, head_dim]")
    if cos.ndim != 2 or sin.ndim != 2:
        raise ValueError(f"{name} expects 2D cos, sin [seq_len, head_dim]")
    S, Hq, D = q.shape
    if k.shape[0] != S or k.shape[2] != D or cos.shape != (S, D) or sin.shape != (S, D):
        raise ValueError(f"{name}: shape mismatch q{q.shape} k{k.shape} cos{cos.shape} sin{sin.shape}")
    if k.dtype != q.dtype:
        raise ValueError(f"{name}: q and k dtypes differ")
    want = float32 if f32_table else q.dtype
    if cos.dtype != want or sin.dtype != want:
        raise ValueError(f"{name}: cos/sin must be {want}")
    call("pgk_rope_inplace", q._p, k._p, cos._p, sin._p, S, Hq, k.shape[1], D, q.dtype.code, int(f32_table), None)


def rope_inplace(q: GPUArray, k: GPUArray, cos: GPUArray, sin: GPUArray) -> None:
    _rope(q, k, cos, sin, False, "rope_inplace")


def rope_inplace_f32table(q: GPUArray, k: GPUArray, cos: GPUArray, sin: GPUArray) -> None:
    """bf16/f16 q,k with fp32 tables (no table rounding)."""
    _rope(q, k, cos, sin, True, "rope_inplace_f32table")


# ---- RoPE scaling tables ---------------------------------------------------------------------------------------------

_LAYOUTS = ("interleaved", "half")


def _check_table(max_seq_len: int, head_dim: int, name: str, scale: float = 1.0, layout: str = "interleaved") -> None:
    if head_dim <= 0 or head_dim % 2:
        raise ValueError(f"{name}: head_dim must be positive and even, got {head_dim}")
    if max_seq_len < 1:
        raise ValueError(f"{name}: max_seq_len must be >= 1, got {max_seq_len}")
    if not scale > 0:
        raise ValueError(f"{name}: scale must be positive, got {scale}")
    if layout not in _LAYOUTS:
        raise ValueError(f"{name}: layout must be one of {_LAYOUTS}, got {layout!r}")


def _inv_freq(head_dim: int, base: float) -> np.ndarray:
    half = head_dim // 2
    return 1.0 / (base ** (np.arange(0, half, dtype=np.float32) / half))


def _cos_sin(positions: np.ndarray, inv_freq: np.ndarray, layout: str) -> tuple[np.ndarray, np.ndarray]:
    """fp32 [S, D] tables of outer(positions, inv_freq): "interleaved" [c0, c0, c1, c1, ...] (the reference's), "half"
    [c0 .. c_{h-1}, c0 .. c_{h-1}] (what rope_inplace here reads: rotate-half, columns d < D/2)."""
    angles = np.outer(positions, inv_freq)
    cos_half, sin_half = np.cos(angles), np.sin(angles)
    if layout == "half":
        return np.concatenate([cos_half, cos_half], axis=-1), np.concatenate([sin_half, sin_half], axis=-1)
    return np.repeat(cos_half, 2, axis=-1), np.repeat(sin_half, 2, axis=-1)


def rope_init_ntk_aware_host(max_seq_len: int, head_dim: int, base: float = 10000.0, scale: float = 1.0, *,
                             layout: str = "interleaved") -> tuple[np.ndarray, np.ndarray]:
    _check_table(max_seq_len, head_dim, "rope_init_ntk_aware", scale, layout)
    if scale > 1.0 and head_dim == 2:
        raise ValueError("rope_init_ntk_aware: head_dim 2 has no NTK exponent (head_dim / (head_dim - 2))")
    scaled_base = base * (scale ** (head_dim / (head_dim - 2))) if scale > 1.0 else base
    return _cos_sin(np.arange(max_seq_len, dtype=np.float32), _inv_freq(head_dim, scaled_base), layout)


def rope_init_linear_host(max_seq_len: int, head_dim: int, base: float = 10000.0, scale: float = 1.0, *,
                          layout: str = "interleaved") -> tuple[np.ndarray, np.ndarray]:
    _check_table(max_seq_len, head_dim, "rope_init_linear", scale, layout)
    return _cos_sin(np.arange(max_seq_len, dtype=np.float32) / scale, _inv_freq(head_dim, base), layout)


def rope_init_yarn_host(max_seq_len: int, head_dim: int, base: float = 10000.0, scale: float = 1.0, original_max_len: int = 4096,
                        beta_fast: float = 32.0, beta_slow: float = 1.0, mscale: float = 0.1, *,
                        layout: str = "interleaved") -> tuple[np.ndarray, np.ndarray]:
    _check_table(max_seq_len, head_dim, "rope_init_yarn", scale, layout)
    inv_freq = _inv_freq(head_dim, base)
    wavelengths = 2 * np.pi / inv_freq
    low_freq_wavelen = original_max_len / beta_slow
    high_freq_wavelen = original_max_len / beta_fast
    smooth = np.clip((wavelengths - high_freq_wavelen) / (low_freq_wavelen - high_freq_wavelen), 0, 1)
    scaled_inv_freq = inv_freq / scale
    interpolated = (1 - smooth) * scaled_inv_freq + smooth * inv_freq
    cos, sin = _cos_sin(np.arange(max_seq_len, dtype=np.float32), interpolated, layout)
    if mscale > 0:          # the reference's device kernel; its CPU path drops mscale
        factor = np.float32(mscale * math.log(scale) + 1.0)
        cos, sin = cos * factor, sin * factor
    return cos, sin


def pope_init_encoding_host(max_seq_len: int, head_dim: int, base: float = 10000.0) -> np.ndarray:
    _check_table(max_seq_len, head_dim, "pope_init_encoding")
    angles = np.outer(np.arange(max_seq_len, dtype=np.float32), _inv_freq(head_dim, base))
    encoding = np.zeros((max_seq_len, head_dim), dtype=np.float32)
    encoding[:, 0::2] = np.sin(angles)
    encoding[:, 1::2] = np.cos(angles)
    return encoding


def alibi_init_slopes_host(num_heads: int) -> np.ndarray:
    if num_heads < 1:
        raise ValueError(f"alibi_init_slopes: num_heads must be >= 1, got {num_heads}")
    return np.array([2 ** (-8 * (h + 1) / num_heads) for h in range(num_heads)], dtype=np.float32)


def _upload(tables) -> tuple[GPUArray, GPUArray]:
    return tuple(from_numpy(np.ascontiguousarray(t, np.float32)) for t in tables)


def rope_init_ntk_aware(max_seq_len: int, head_dim: int, base: float = 10000.0, scale: float = 1.0, *,
                        layout: str = "interleaved") -> tuple[GPUArray, GPUArray]:
    """(cos, sin) fp32 [max_seq_len, head_dim] with the base scaled: base * scale ** (head_dim / (head_dim - 2)) for
    scale > 1, the plain base otherwise.  [build-defined] layout="half" gives the tables rope_inplace here reads."""
    return _upload(rope_init_ntk_aware_host(max_seq_len, head_dim, base, scale, layout=layout))


def rope_init_yarn(max_seq_len: int, head_dim: int, base: float = 10000.0, scale: float = 1.0, original_max_len: int = 4096,
                   beta_fast: float = 32.0, beta_slow: float = 1.0, mscale: float = 0.1, *,
                   layout: str = "interleaved") -> tuple[GPUArray, GPUArray]:
    """(cos, sin) fp32 [max_seq_len, head_dim] with the reference's wavelength ramp between original_max_len / beta_fast and
    original_max_len / beta_slow, both tables times float32(mscale * ln(scale) + 1) when mscale > 0.  The ramp divides the
    SHORT wavelengths by `scale` - the opposite of the published YaRN."""
    return _upload(rope_init_yarn_host(max_seq_len, head_dim, base, scale, original_max_len, beta_fast, beta_slow, mscale, layout=layout))


def rope_init_linear(max_seq_len: int, head_dim: int, base: float = 10000.0, scale: float = 1.0, *,
                     layout: str = "interleaved") -> tuple[GPUArray, GPUArray]:
    """(cos, sin) fp32 [max_seq_len, head_dim] at positions arange(S) / scale (linear position interpolation)."""
    return _upload(rope_init_linear_host(max_seq_len, head_dim, base, scale, layout=layout))


# ---- PoPE ------------------------------------------------------------------------------------------------------------

def pope_init_encoding(max_seq_len: int, head_dim: int, base: float = 10000.0) -> GPUArray:
    """fp32 [max_seq_len, head_dim]: even columns sin, odd columns cos of pos / base ** (2i / head_dim)."""
    return from_numpy(pope_init_encoding_host(max_seq_len, head_dim, base))


def pope_inplace(q: GPUArray, k: GPUArray, encoding: GPUArray, start_pos: int = 0) -> None:
    """q [S, Hq, D], k [S, Hk, D] += encoding[start_pos + s] (fp32 [max_seq, D]): one fp32 add, one rounding to q's dtype."""
    validate_float(q, "pope_inplace")
    if q.ndim != 3 or k.ndim != 3:
        raise ValueError("pope_inplace expects 3D q, k [seq_len, n_heads, head_dim]")
    S, Hq, D = q.shape
    if k.shape[0] != S or k.shape[2] != D:
        raise ValueError(f"pope_inplace: shape mismatch q{q.shape} k{k.shape}")
    if k.dtype != q.dtype:
        raise ValueError("pope_inplace: q and k dtypes differ")
    if encoding.dtype != float32 or encoding.ndim != 2 or encoding.shape[1] != D:
        raise ValueError(f"pope_inplace: encoding must be float32 [max_seq, {D}], got {encoding.dtype} {encoding.shape}")
    if start_pos < 0 or start_pos + S > encoding.shape[0]:
        raise ValueError(f"pope_inplace: rows {start_pos}..{start_pos + S} outside the encoding table of {encoding.shape[0]} rows")
    call("pgk_pope_inplace", q._p, k._p, encoding._p, S, Hq, k.shape[1], D, int(start_pos), encoding.shape[0], q.dtype.code, None)


# ---- ALiBi -----------------------------------------------------------------------------------------------------------

def alibi_init_slopes(num_heads: int) -> GPUArray:
    """fp32 [num_heads]: float32(2 ** (-8 * (h + 1) / num_heads))."""
    return from_numpy(alibi_init_slopes_host(num_heads))


def _check_slopes(slopes: GPUArray, num_heads: int, name: str) -> None:
    if slopes.dtype != float32:
        raise ValueError(f"{name}: slopes must be float32, got {slopes.dtype}")
    if slopes.size != num_heads:
        raise ValueError(f"{name}: slopes must have {num_heads} elements, got shape {slopes.shape}")


def alibi_compute_bias(seq_len: int, num_heads: int, slopes: GPUArray, causal: bool = True) -> GPUArray:
    """fp32 [num_heads, seq_len, seq_len]: -slope * (i - j); above the diagonal -1e9 when causal, else the same product
    (positive, as the reference's CPU path).  Attention itself never needs this tensor: sdpa_alibi."""
    if seq_len < 1 or num_heads < 1:
        raise ValueError(f"alibi_compute_bias: needs seq_len >= 1 and num_heads >= 1, got {seq_len}, {num_heads}")
    _check_slopes(slopes, num_heads, "alibi_compute_bias")
    bias = GPUArray((num_heads, seq_len, seq_len), float32)
    call("pgk_alibi_compute_bias", slopes._p, bias._p, seq_len, num_heads, int(bool(causal)), None)
    return bias


def alibi_add_bias(scores: GPUArray, slopes: GPUArray, start_pos: int = 0) -> None:
    """scores fp32 [batch, num_heads, q_len, kv_len] -= slope[h] * (start_pos + i - j), every j, in place."""
    if scores.dtype != float32:
        raise ValueError(f"alibi_add_bias: scores must be float32, got {scores.dtype}")
    if scores.ndim != 4:
        raise ValueError(f"alibi_add_bias expects 4D scores [batch, num_heads, q_len, kv_len], got {scores.ndim}D")
    b, h, q_len, kv_len = scores.shape
    _check_slopes(slopes, h, "alibi_add_bias")
    call("pgk_alibi_add_bias", scores._p, slopes._p, b, h, q_len, kv_len, int(start_pos), scores.dtype.code, slopes.dtype.code,
         slopes.size, None)


__all__ = ["rope_inplace", "rope_inplace_f32table", "rope_init_ntk_aware", "rope_init_yarn", "rope_init_linear",
           "pope_init_encoding", "pope_inplace", "alibi_init_slopes", "alibi_compute_bias", "alibi_add_bias"]
