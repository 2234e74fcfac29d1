"""[build-defined] Restated oracle of the fp8-in / fp8-out GEMMs (matmul_fp8_fp8_sm120 and
matmul_fp8_fp8_blockwise_sm120, reference src/pygpukit/ops/matmul/fp8.py:220-343).  Their native side is CUTLASS
and absent from the reference checkout, so the contract is the formula of include/pgk_hip.h
(pgk_gemm_fp8_fp8_nn):

    D[m][n] = e4m3( sum_kb sA(m/128, kb) * sB(n/128, kb) * sum_{k in kb} A[m][k] * B[k][n] )

A [M,K], B [K,N], D [M,N] e4m3 codes; scales fp32, MN-major (element (mb, kb) of scale_a at kb*ceil(M/128) + mb,
(nb, kb) of scale_b at kb*ceil(N/128) + nb: CUTLASS's Sm1xxBlockwiseScaleConfig default, not pinned by a
reference run).  The product is evaluated in float64 and rounded to fp32, then encoded with round-to-nearest-even
and satfinite (CUTLASS float_e4m3_t): |x| > 448 -> +-448, NaN stays a NaN code, -0 -> 0x80."""

from __future__ import annotations

import numpy as np

from oracle import cpu_ref as O


def e4m3_satfinite_codes(x) -> np.ndarray:
    """fp32 -> OCP e4m3 code: RNE, finite values beyond 448 (and +-inf) saturate to 0x7E / 0xFE, NaN -> 0x7F / 0xFF
    (sign kept), -0 -> 0x80.  oracle.cpu_ref._rne_e4m3_codes alone maps NaN to a finite code."""
    x = np.asarray(x, np.float32)
    codes = O._rne_e4m3_codes(np.where(np.isnan(x), np.float32(0.0), x))
    nan = np.where(np.signbit(x), np.uint8(0xFF), np.uint8(0x7F))
    return np.where(np.isnan(x), nan, codes).astype(np.uint8)


def scale_sizes(M: int, N: int, K: int) -> tuple[int, int]:
    kb = (K + 127) // 128
    return ((M + 127) // 128) * kb, ((N + 127) // 128) * kb


def expand_scales(scale, rows: int, K: int) -> np.ndarray:
    """MN-major block scales (ceil(rows/128)*ceil(K/128) elements) -> float64 [rows, K], one value per element."""
    rb, kb = (rows + 127) // 128, (K + 127) // 128
    s = np.asarray(scale, np.float64).reshape(kb, rb).T            # [rb, kb]
    return np.repeat(np.repeat(s, 128, axis=0), 128, axis=1)[:rows, :K]


def gemm_fp8_fp8_nn_f32(a_codes, b_codes, scale_a=None, scale_b=None) -> np.ndarray:
    """The fp32 product before the output rounding: float64 sum, rounded once to fp32.  An exact zero is +0 (the
    kernel's sums start from +0)."""
    table = O.fp8_e4m3_table().astype(np.float64)
    a = table[np.asarray(a_codes)]
    b = table[np.asarray(b_codes)]
    M, K = a.shape
    N = b.shape[1]
    if scale_a is not None:
        a = a * expand_scales(scale_a, M, K)
        b = b * expand_scales(scale_b, N, K).T
    return (a @ b).astype(np.float32) + np.float32(0.0)


def gemm_fp8_fp8_nn(a_codes, b_codes, scale_a=None, scale_b=None) -> np.ndarray:
    """D codes uint8 [M,N]."""
    return e4m3_satfinite_codes(gemm_fp8_fp8_nn_f32(a_codes, b_codes, scale_a, scale_b))


def quantize_blocks(x: np.ndarray, extra: float = 1.0):
    """Per 128x128 block of a float [R,K] array: scale = absmax/448 (1 for an all-zero block), codes = RNE e4m3 of
    x/scale.  Returns (codes uint8 [R,K], scale fp32 MN-major, times `extra`)."""
    R, K = x.shape
    rb, kb = (R + 127) // 128, (K + 127) // 128
    xp = np.zeros((rb * 128, kb * 128), np.float32)
    xp[:R, :K] = x
    amax = np.abs(xp.reshape(rb, 128, kb, 128)).max(axis=(1, 3))    # [rb, kb]
    s = np.where(amax > 0, amax / np.float32(448.0), np.float32(1.0)).astype(np.float32)
    q = (xp / np.repeat(np.repeat(s, 128, axis=0), 128, axis=1)).astype(np.float32)
    codes = O._rne_e4m3_codes(q)[:R, :K]
    return np.ascontiguousarray(codes), np.ascontiguousarray((s * np.float32(extra)).T.reshape(-1)).astype(np.float32)


def code_ordinal(codes) -> np.ndarray:
    """Signed position on the e4m3 number line (+0 and -0 both 0): one e4m3 step apart = ordinals 1 apart."""
    c = np.asarray(codes).astype(np.int32)
    return np.where(c & 0x80, -(c & 0x7F), c & 0x7F)
