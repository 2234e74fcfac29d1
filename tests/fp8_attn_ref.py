"""[build-defined] Restated oracle of sdpa_causal_fp8 (reference src/pygpukit/ops/nn/attention.py:238-347, native
flash_attention_3_fp8_sm120.cuh).  The reference's kernel needs another vendor's instruction set, so the contract is
the formula of include/pgk_hip.h (pgk_sdpa_causal_fp8, pgk_quantize_fp8_per_head):

  per head of Q and per kv head of K:   a = max|X_h|;  e = 0 if a == 0 else the smallest integer with 448 * 2^e >= a,
      clamped to [-127, 127];  scale byte = e + 127 (UE8M0);  code = e4m3(X * 2^-e), RNE, satfinite
  s[i][j] = scale * 2^(eq + ek) * sum_d T[qc[i][d]] * T[kc[j][d]]   (scale <= 0 -> 1/sqrt(128)),  mask j <= (kv - q) + i
  out = softmax(s) . V     with V unquantised

All arithmetic after the quantisation is float64 (oracle.cpu_ref.sdpa_causal on the dequantised operands)."""

from __future__ import annotations

import numpy as np

from oracle import cpu_ref as O
from tests.fp8_io_ref import e4m3_satfinite_codes


def head_exponent(absmax: float) -> int:
    """Smallest integer e with 448 * 2^e >= absmax (exact: powers of two times 448 in float64), clamped; 0 for 0."""
    a = float(absmax)
    if a == 0.0:
        return 0
    m, x = np.frexp(a / 448.0)                 # a / 448 = m * 2^x, 0.5 <= m < 1: a / 448 is exact to 53 bits for bf16 a
    e = int(x) - 1 if m == 0.5 else int(x)     # ceil(log2(a / 448)) without libm
    assert 448.0 * 2.0 ** e >= a and 448.0 * 2.0 ** (e - 1) < a
    return max(-127, min(127, e))


def quantize_per_head(x: np.ndarray):
    """x float [H, rows, D] (bf16 values) -> (codes uint8 [H, rows, D], scale_bytes uint8 [H])."""
    x = np.asarray(x, np.float32)
    codes = np.empty(x.shape, np.uint8)
    sb = np.empty(x.shape[0], np.uint8)
    for h in range(x.shape[0]):
        e = head_exponent(np.abs(x[h]).max())
        sb[h] = e + 127
        codes[h] = e4m3_satfinite_codes((x[h].astype(np.float64) * 2.0 ** (-e)).astype(np.float32))
    return codes, sb


def dequantize_per_head(codes: np.ndarray, scale_bytes: np.ndarray) -> np.ndarray:
    t = O.fp8_e4m3_table().astype(np.float64)
    return t[codes] * (2.0 ** (scale_bytes.astype(np.float64) - 127.0))[:, None, None]


def sdpa_causal_fp8(q: np.ndarray, k: np.ndarray, v: np.ndarray, scale: float = 0.0) -> np.ndarray:
    """q [Hq, q_len, 128], k / v [Hkv, kv_len, 128] float arrays holding bf16 values -> float64 [Hq, q_len, 128]."""
    rep = q.shape[0] // k.shape[0]
    qd = dequantize_per_head(*quantize_per_head(q))
    kd = np.repeat(dequantize_per_head(*quantize_per_head(k)), rep, axis=0)     # per kv head == per expanded head
    vd = np.repeat(np.asarray(v, np.float64), rep, axis=0)
    return O.sdpa_causal(qd, kd, vd, float(scale))


def sdpa_causal_unquantised(q, k, v, scale: float = 0.0) -> np.ndarray:
    rep = q.shape[0] // k.shape[0]
    f = lambda a: np.asarray(a, np.float64)    # noqa: E731
    return O.sdpa_causal(f(q), np.repeat(f(k), rep, axis=0), np.repeat(f(v), rep, axis=0), float(scale))


def bf16_normal(rng, shape) -> np.ndarray:
    """Standard-normal data rounded to bf16, as fp32."""
    return O.bf16_round(rng.standard_normal(shape).astype(np.float32))


def exact_integer_qk(rng, hq, hkv, q_len, kv_len):
    """Q, K random integers in [-15, 15] with +-15 planted in every head (head exponent -4): every value is a 4-bit
    significand and survives the quantisation exactly.  V standard normal."""
    q = rng.integers(-15, 16, (hq, q_len, 128)).astype(np.float32)
    k = rng.integers(-15, 16, (hkv, kv_len, 128)).astype(np.float32)
    q[:, 0, 0], k[:, 0, 0] = 15.0, -15.0
    return q, k, bf16_normal(rng, (hkv, kv_len, 128))
