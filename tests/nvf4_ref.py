"""NumPy restatement of the NVF4 ops (reference: native/ops/matmul/gemv/w4a16_bf16/sm120/nvf4.cuh:36-110,
nvf4_kernels.cu:19-345, native/ops/matmul/gemm/w4a16_bf16/sm120/nvf4_cutlass.cu:157-317), in float32 step by step.

  quantize_nvf4(x [K,N])     -> data uint8 [K/2, N], scale uint8 [ceil(K/32), N]
  gemv_nvf4(a, data, scale)  -> C[n] = bf16(alpha * sum_k a[k] * lut[code] * scale), accumulated in float64 (exact
                                for the exact-data tests; the random-data tests compare within a tolerance)
  gemm_nvf4(a, b)            -> D = bf16(e2m1(a) @ e2m1(b)), unit scales, exact

The weight quantiser keeps one detail of the reference that a prose description easily drops: the doubling loop
for a scale below 1 only runs when the scale is above 1e-8 (nvf4_kernels.cu:275), so a block whose max|x| lies in
(1e-8, 6e-8] keeps exponent 0 and gets scale byte 0x38."""

from __future__ import annotations

import numpy as np

from oracle import cpu_ref as O

E2M1 = np.array([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6], np.float32)
THRESH = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], np.float32)
F32 = np.float32


def scale_value(s) -> np.ndarray:
    """Scale byte -> float32: (1 + (s&7)/8) * 2^(((s>>3)&15) - 7); bit 7 ignored."""
    s = np.asarray(s).astype(np.int64)
    return ((1 + (s & 7) / 8) * np.exp2(((s >> 3) & 15) - 7)).astype(np.float32)


def code_scaled(v: np.ndarray) -> np.ndarray:
    """The quantiser's `<` chain (nvf4_kernels.cu:296-307): sign (v < 0) | the number of thresholds |v| is not below.
    NaN is below none of them: code 7 (+6)."""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        a = np.abs(v)
        c = sum((~(a < t)).astype(np.uint8) for t in THRESH)
        return (np.where(v < 0, 8, 0) | c).astype(np.uint8)


def e2m1_unit(x: np.ndarray) -> np.ndarray:
    """bf16_to_nvf4_e2m1 (nvf4_cutlass.cu:160-176): sign (x < 0) | the number of thresholds |x| reaches (>=).
    NaN reaches none: +0.  +-inf -> +-6."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        a = np.abs(x)
        c = sum((a >= t).astype(np.uint8) for t in THRESH)
        return (np.where(x < 0, 8, 0) | c).astype(np.uint8)


def scale_byte(max_abs: np.ndarray) -> np.ndarray:
    """Per-block scale byte from the block's max|x| (nvf4_kernels.cu:258-289), float32 throughout."""
    max_abs = np.asarray(max_abs, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.where(max_abs > F32(1e-8), max_abs / F32(6), F32(1)).astype(np.float32)
        e = np.zeros(s.shape, np.int64)
        norm = s.copy()
        up = norm >= F32(2)
        down = ~up & (norm < F32(1)) & (norm > F32(1e-8))
        for _ in range(8):
            m = up & (norm >= F32(2)) & (e < 8)
            norm = np.where(m, norm * F32(0.5), norm).astype(np.float32)
            e += m
        for _ in range(7):
            m = down & (norm < F32(1)) & (e > -7)
            norm = np.where(m, norm * F32(2), norm).astype(np.float32)
            e -= m
        mant = np.clip(np.rint((norm - F32(1)) * F32(8)), 0, 7).astype(np.int64)   # no carry into the exponent
    eb = np.clip(e + 7, 0, 15)
    return ((eb << 3) | mant).astype(np.uint8)


def quantize_nvf4(x: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """x float32 [K, N] (bf16 values), K even -> (data [K/2, N], scale [ceil(K/32), N])."""
    x = np.asarray(x, np.float32)
    K, N = x.shape
    assert K % 2 == 0
    nsb = (K + 31) // 32
    data = np.zeros((K // 2, N), np.uint8)
    scale = np.zeros((nsb, N), np.uint8)
    for sb in range(nsb):
        blk = x[sb * 32:min(sb * 32 + 32, K)]
        max_abs = np.fmax.reduce(np.abs(blk), axis=0, initial=F32(0)).astype(np.float32)   # NaN ignored
        sbyte = scale_byte(max_abs)
        scale[sb] = sbyte
        inv = (F32(1) / scale_value(sbyte)).astype(np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            codes = code_scaled((blk * inv).astype(np.float32))
        data[sb * 16:sb * 16 + codes.shape[0] // 2] = codes[0::2] | (codes[1::2] << 4)
    return data, scale


def dequant(data: np.ndarray, scale: np.ndarray, K: int) -> np.ndarray:
    """[K, N] float32 lut[code] * scale (exact)."""
    data = np.asarray(data, np.uint8)
    N = data.shape[1]
    codes = np.empty((K, N), np.uint8)
    codes[0::2] = data[:K // 2] & 15
    codes[1::2] = data[:K // 2] >> 4
    s = scale_value(np.asarray(scale, np.uint8).reshape(-1)[:((K + 31) // 32) * N].reshape(-1, N))
    return E2M1[codes] * np.repeat(s, 32, axis=0)[:K]


def _gemv_sum(a: np.ndarray, data: np.ndarray, scale: np.ndarray) -> np.ndarray:
    """a @ dequant in float64, 2048 columns at a time (exact for the exact-data tests)."""
    a = np.asarray(a, np.float64)
    K, N = a.shape[0], data.shape[1]
    nsb = (K + 31) // 32
    scale = np.asarray(scale, np.uint8).reshape(-1)[:nsb * N].reshape(nsb, N)
    return np.concatenate([a @ dequant(data[:, n:n + 2048], scale[:, n:n + 2048], K).astype(np.float64)
                           for n in range(0, N, 2048)])


def gemv_nvf4_f64(a: np.ndarray, data: np.ndarray, scale: np.ndarray, alpha: float = 1.0) -> np.ndarray:
    """alpha * a @ dequant in float64 (no rounding)."""
    return float(alpha) * _gemv_sum(a, data, scale)


def gemv_nvf4(a: np.ndarray, data: np.ndarray, scale: np.ndarray, alpha: float = 1.0) -> np.ndarray:
    """bf16 bits of C = bf16(fp32(alpha) * fp32(sum)), the sum taken exactly (float64)."""
    s = _gemv_sum(a, data, scale).astype(np.float32)
    return O.f32_to_bf16_bits((F32(alpha) * s).astype(np.float32))


def gemm_nvf4(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """bf16 bits of D = e2m1(a) @ e2m1(b) (unit scales; exact in float64, hence in fp32 for K < 116000)."""
    av = E2M1[e2m1_unit(a)].astype(np.float64)
    bv = E2M1[e2m1_unit(b)].astype(np.float64)
    return O.f32_to_bf16_bits((av @ bv).astype(np.float32))
