"""CPU checks of the NVF4 surface: the reference's names and aliases, the size helper, and the restated oracle
(tests/nvf4_ref.py) on hand-worked cases - scale bytes, every threshold tie, NaN / inf in both quantisers, the bit-7
mirror of scale bytes and a short tail block."""

from __future__ import annotations

import importlib

import numpy as np
import pytest

from tests import nvf4_ref as R

NAMES = ["nvf4_get_sizes", "gemv_nvf4_get_sizes", "quantize_bf16_to_nvf4", "matmul_nvf4_bf16_sm120", "gemm_nvf4_bf16_sm120",
         "gemv_nvf4_bf16", "gemv_nvf4_bf16_sm120", "nvf4_bf16_sm120_available", "gemm_nvf4_bf16_sm120_available",
         "gemv_nvf4_available", "gemv_nvf4_bf16_sm120_available"]


@pytest.mark.parametrize("module", ["pygpukit_amd.ops.matmul", "pygpukit_amd.ops", "pygpukit_amd.ops.matmul.nvf4"])
def test_reference_names_and_aliases(module):
    mod = importlib.import_module(module)
    missing = [n for n in NAMES if not hasattr(mod, n)]
    assert not missing, missing
    assert mod.gemv_nvf4_get_sizes is mod.nvf4_get_sizes
    assert mod.gemm_nvf4_bf16_sm120 is mod.matmul_nvf4_bf16_sm120
    assert mod.gemv_nvf4_bf16_sm120 is mod.gemv_nvf4_bf16
    assert mod.gemm_nvf4_bf16_sm120_available is mod.nvf4_bf16_sm120_available
    assert mod.gemv_nvf4_bf16_sm120_available is mod.gemv_nvf4_available
    assert mod.nvf4_bf16_sm120_available() is True and mod.gemv_nvf4_available() is True
    from pygpukit_amd.ops.matmul import nvf4

    assert set(NAMES) <= set(nvf4.__all__)


def test_get_sizes():
    from pygpukit_amd.ops import nvf4_get_sizes

    assert nvf4_get_sizes(4096, 14336) == (2048 * 14336, 128 * 14336)
    assert nvf4_get_sizes(66, 333) == (33 * 333, 3 * 333)
    assert nvf4_get_sizes(1000, 1) == (500, 32)
    assert nvf4_get_sizes(32, 7) == (112, 7)


def test_new_entry_points_declared():
    from pygpukit_amd import _hip

    for name in ("pgk_quantize_nvf4", "pgk_gemv_nvf4_bf16", "pgk_quantize_e2m1_unit", "pgk_gemm_fp4_nt",
                 "pgk_gemv_nvf4_workspace_bytes", "pgk_gemm_nvf4_workspace_bytes"):
        assert name in _hip.EXPORTED_SYMBOLS


@pytest.mark.parametrize("max_abs, byte", [
    (6.0, 0x38),           # scale 1: exponent 0 -> field 7, mantissa 0
    (0.0, 0x38),           # all-zero block: scale 1
    (12.0, 0x40),          # scale 2: field 8
    (3.0, 0x30),           # scale 0.5: field 6
    (6.375, 0x38),         # scale 1.0625: (0.0625 * 8) = 0.5 rounds to even 0
    (7.125, 0x3A),         # scale 1.1875: 1.5 rounds to even 2
    (11.9375, 0x3F),       # scale 1.9896: mantissa rounds to 8, clamps to 7, no carry into the exponent
    (2.0 ** -10, 0x00),    # tiny: the doubling stops at exponent -7, mantissa clamps to 0
    (3e-8, 0x38),          # scale 5e-9 <= 1e-8: the reference does not normalise it (exponent 0, mantissa 0)
    (5e-9, 0x38),          # max|x| <= 1e-8: scale 1
    (6000.0, 0x7F),        # huge: the halving stops at exponent 8, mantissa clamps to 7
    (np.inf, 0x7F),
])
def test_scale_bytes(max_abs, byte):
    assert int(R.scale_byte(np.float32(max_abs))) == byte
    x = np.zeros((32, 1), np.float32)
    x[5, 0] = max_abs
    x[9, 0] = -max_abs / 2
    _, scale = R.quantize_nvf4(x)
    assert int(scale[0, 0]) == byte


def test_scale_value_and_bit7_mirror():
    s = np.arange(256)
    v = R.scale_value(s)
    np.testing.assert_array_equal(v[128:], v[:128])
    assert v[0x38] == 1.0 and v[0x00] == 2.0 ** -7 and v[0x7F] == 480.0 and v[0x3C] == 1.5
    assert np.all(np.diff(v[:128]) > 0)


def _ties():
    t = R.THRESH
    below = np.nextafter(t, np.float32(0))
    return np.concatenate([t, below, -t, -below]).astype(np.float32)


def test_every_threshold_tie_weight_quantiser():
    """Scale 1 (the block's max is 6): v = x exactly; ties go up in magnitude, just below stays down."""
    v = _ties()
    want = np.concatenate([np.arange(1, 8), np.arange(0, 7), 8 | np.arange(1, 8), 8 | np.arange(0, 7)]).astype(np.uint8)
    np.testing.assert_array_equal(R.code_scaled(v), want)
    x = np.zeros((32, 1), np.float32)
    x[:28, 0] = v[:28]
    x[28, 0] = 6.0
    data, scale = R.quantize_nvf4(x)
    assert scale[0, 0] == 0x38
    codes = np.empty(32, np.uint8)
    codes[0::2], codes[1::2] = data[:, 0] & 15, data[:, 0] >> 4
    np.testing.assert_array_equal(codes[:28], want[:28])
    assert codes[28] == 7


def test_every_threshold_tie_unit_quantiser():
    v = _ties()
    want = np.concatenate([np.arange(1, 8), np.arange(0, 7), 8 | np.arange(1, 8), 8 | np.arange(0, 7)]).astype(np.uint8)
    np.testing.assert_array_equal(R.e2m1_unit(v), want)
    assert list(R.e2m1_unit(np.array([0.0, -0.0, 6.0, 5.5, 100.0, -7.0], np.float32))) == [0, 0, 7, 7, 7, 15]


def test_nan_and_inf():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    # the unit quantiser: NaN -> +0 (reaches no threshold), +-inf -> +-6
    assert list(R.e2m1_unit(np.array([nan, -nan, inf, -inf], np.float32))) == [0, 0, 7, 15]
    # the weight quantiser: NaN is skipped by the max and coded 7 (+6)
    x = np.zeros((32, 3), np.float32)
    x[0, 0], x[1, 0], x[2, 0] = nan, 6.0, -1.0
    x[0, 1], x[1, 1], x[2, 1], x[3, 1] = inf, -inf, 480.0, -1000.0
    x[0, 2] = -nan
    data, scale = R.quantize_nvf4(x)
    assert list(scale[0]) == [0x38, 0x7F, 0x38]
    assert data[0, 0] == (7 | (7 << 4)) and data[1, 0] == 10
    # scale 480: inf -> 7, -inf -> 15, 480 / 480 = 1 -> 2, -1000/480 = -2.08 -> 12
    assert data[0, 1] == (7 | (15 << 4)) and data[1, 1] == (2 | (12 << 4))
    assert data[0, 2] & 15 == 7


def test_short_tail_block_and_layout():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((34, 5)).astype(np.float32)
    x[32:, 1] = 0.0
    data, scale = R.quantize_nvf4(x)
    assert data.shape == (17, 5) and scale.shape == (2, 5)
    assert scale[1, 1] == 0x38
    # the tail block's scale comes from rows 32..33 only
    np.testing.assert_array_equal(scale[1], R.scale_byte(np.abs(x[32:]).max(axis=0)))
    # the dequantised tail is within half a step of x
    deq = R.dequant(data, scale, 34)
    s = R.scale_value(scale[1])
    assert np.all(np.abs(deq[32:] - x[32:]) <= s * 1.0 + 1e-6)


def test_gemv_oracle_matches_dequant_product():
    rng = np.random.default_rng(1)
    K, N = 66, 7
    data = rng.integers(0, 256, (K // 2, N)).astype(np.uint8)
    scale = rng.integers(0, 256, (3, N)).astype(np.uint8)
    a = rng.integers(-3, 4, K).astype(np.float32)
    lut = R.E2M1
    want = np.zeros(N)
    for n in range(N):
        for k in range(K):
            code = (data[k // 2, n] >> (4 * (k & 1))) & 15
            want[n] += a[k] * lut[code] * R.scale_value(scale[k // 32, n])
    np.testing.assert_array_equal(R.gemv_nvf4_f64(a, data, scale), want)


def test_gemm_oracle_small():
    a = np.array([[0.3, -1.3, np.nan, 7.0]], np.float32)           # codes 1, 11, 0, 7 -> .5, -1.5, 0, 6
    b = np.array([[1.0], [2.0], [3.0], [-0.7]], np.float32)        # 2, 4, 5, 9 -> 1, 2, 3, -.5
    from oracle import cpu_ref as O

    assert O.bf16_bits_to_f32(R.gemm_nvf4(a, b))[0, 0] == np.float32(0.5 - 3.0 - 3.0)
