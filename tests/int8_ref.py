"""Oracle of the integer family (pygpukit_amd.ops.matmul.int8, pygpukit_amd.ops.quantize): int64 products, the quantiser and
the scale epilogues restated in float32 step by step, float64 for the 16-bit linears, and the nibble pack / unpack helpers."""

from __future__ import annotations

import numpy as np

F32 = np.float32


# ---- storage -------------------------------------------------------------------------------------------------------------------
def pack_int4(v: np.ndarray) -> np.ndarray:
    """[..., K] integers in -8..7 -> [..., K/2] uint8, k even in the low nibble, k + 1 in the high one."""
    v = np.asarray(v)
    assert v.shape[-1] % 2 == 0 and v.min() >= -8 and v.max() <= 7
    u = (v & 0xF).astype(np.uint8)
    return (u[..., 0::2] | (u[..., 1::2] << 4)).astype(np.uint8)


def unpack_int4(p: np.ndarray) -> np.ndarray:
    p = np.asarray(p, np.uint8)
    out = np.empty(p.shape[:-1] + (p.shape[-1] * 2,), np.int8)
    out[..., 0::2] = (p << 4).astype(np.int8) >> 4
    out[..., 1::2] = p.astype(np.int8) >> 4
    return out


def bf16_bits(x: np.ndarray) -> np.ndarray:
    """float32 -> bfloat16 bits, round to nearest even."""
    u = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits: np.ndarray) -> np.ndarray:
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(F32)


def to_storage(x: np.ndarray, dtype: str) -> np.ndarray:
    """float32 values -> the host array of a GPUArray of `dtype` (bfloat16 travels as uint16)."""
    return bf16_bits(x) if dtype == "bfloat16" else np.asarray(x, F32).astype({"float32": F32, "float16": np.float16}[dtype])


def from_storage(a: np.ndarray, dtype: str) -> np.ndarray:
    return bf16_value(a) if dtype == "bfloat16" else np.asarray(a).astype(F32)


# ---- integer products -----------------------------------------------------------------------------------------------------------
def gemm_int(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """A [M,K] . B [N,K]^T as int64, the true sum.  The products go through float64 (BLAS): |a b| <= 2^14, so every partial
    sum is an integer below 2^53 and exact for K < 2^39."""
    return np.rint(a.astype(np.float64) @ b.astype(np.float64).T).astype(np.int64)


def wrap_int32(acc: np.ndarray) -> np.ndarray:
    """The int64 sum modulo 2^32 as int32: what an int32 accumulator holds."""
    return np.asarray(acc, np.int64).astype(np.uint64).astype(np.uint32).view(np.int32)


def roundf(r: np.ndarray) -> np.ndarray:
    """C roundf of float32 values: half away from zero (|r| + 0.5 is exact in float64)."""
    r = np.asarray(r, F32).astype(np.float64)
    return (np.sign(r) * np.floor(np.abs(r) + 0.5)).astype(F32)


def scale_round(acc: np.ndarray, factors, out_int8: bool) -> np.ndarray:
    """saturate(roundf((float)acc * f0 * f1 ...)), the products in float32, left to right.  All factors 1.0 and int32 out: the
    accumulator itself."""
    if not out_int8 and all(F32(f) == F32(1.0) for f in factors):
        return wrap_int32(acc)
    r = wrap_int32(acc).astype(F32)
    for f in factors:
        r = (r * F32(f)).astype(F32)
    r = roundf(r).astype(np.float64)
    lo, hi = (-128, 127) if out_int8 else (-2 ** 31, 2 ** 31 - 1)
    return np.clip(r, lo, hi).astype(np.int8 if out_int8 else np.int32)


def gemv_int4(a: np.ndarray, b: np.ndarray, scale_a: float, scale_b: float) -> np.ndarray:
    """a [K], b [N,K] nibble values: the formula is applied as written, unit scales included."""
    r = wrap_int32(b.astype(np.int64) @ a.astype(np.int64)).astype(F32)
    r = ((r * F32(scale_a)).astype(F32) * F32(scale_b)).astype(F32)
    return np.clip(roundf(r).astype(np.float64), -2 ** 31, 2 ** 31 - 1).astype(np.int32)


# ---- quantiser --------------------------------------------------------------------------------------------------------------------
def quantize_rows(x: np.ndarray):
    """x float32 [rows, cols] (values of the input dtype) -> (q int8, s float32 [rows], the UNROUNDED scale)."""
    x = np.asarray(x, F32)
    s = (np.max(np.abs(x), axis=1).astype(F32) / F32(127.0)).astype(F32)
    s = np.maximum(s, F32(1e-10)).astype(F32)
    t = np.rint((x / s[:, None]).astype(F32))          # IEEE division, ties to even
    return np.clip(t, -128, 127).astype(np.int8), s


def dequantize_rows(q: np.ndarray, scale_values: np.ndarray) -> np.ndarray:
    """float32 product of (float)q and the scale's value; the caller rounds once to the output dtype."""
    return (q.astype(F32) * np.asarray(scale_values, F32)[:, None]).astype(F32)


def dequant_gemm_f32(acc: np.ndarray, a_scale: np.ndarray, w_scale: np.ndarray) -> np.ndarray:
    """(float)acc * a_scale[m] * w_scale[n] in float32, left to right."""
    r = (wrap_int32(acc).astype(F32) * a_scale.astype(F32)[:, None]).astype(F32)
    return (r * w_scale.astype(F32)[None, :]).astype(F32)
