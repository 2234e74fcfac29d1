"""CPU checks of the fp8-in / fp8-out GEMM surface: the reference's names are importable, the size helpers follow
their formulas, and the restated oracle (tests/fp8_io_ref.py) encodes e4m3 the way the contract says."""

from __future__ import annotations

import numpy as np
import pytest

from oracle import cpu_ref as O
from tests import fp8_io_ref as R

NAMES = ["matmul_fp8_fp8_sm120", "gemm_fp8_fp8_sm120", "matmul_fp8_fp8_blockwise_sm120", "gemm_fp8_fp8_blockwise_sm120",
         "fp8_fp8_get_scale_sizes", "gemm_fp8_fp8_get_scale_sizes", "fp8_get_sizes", "gemm_fp8_fp8_sm120_available"]


@pytest.mark.parametrize("module", ["pygpukit_amd.ops.matmul", "pygpukit_amd.ops", "pygpukit_amd.ops.matmul.fp8"])
def test_reference_names_import(module):
    import importlib

    mod = importlib.import_module(module)
    missing = [n for n in NAMES if not hasattr(mod, n)]
    assert not missing, missing
    assert mod.gemm_fp8_fp8_sm120 is mod.matmul_fp8_fp8_sm120
    assert mod.gemm_fp8_fp8_blockwise_sm120 is mod.matmul_fp8_fp8_blockwise_sm120
    assert mod.gemm_fp8_fp8_get_scale_sizes is mod.fp8_fp8_get_scale_sizes
    assert mod.gemm_fp8_fp8_sm120_available() is True
    from pygpukit_amd.ops.matmul import fp8

    assert set(NAMES) <= set(fp8.__all__)


@pytest.mark.parametrize("K,N", [(128, 128), (1, 1), (129, 257), (4096, 14336), (400, 208)])
def test_fp8_get_sizes(K, N):
    from pygpukit_amd.ops.matmul import fp8_get_sizes

    sk, sn = -(-K // 128), -(-N // 128)
    assert fp8_get_sizes(K, N) == (sk, sn, sk * sn * 2)


@pytest.mark.parametrize("M,N,K", [(1, 16, 16), (48, 160, 256), (130, 208, 144), (300, 272, 384), (1000, 4096, 4096),
                                   (129, 128, 129)])
def test_fp8_fp8_get_scale_sizes(M, N, K):
    from pygpukit_amd.ops.matmul import fp8_fp8_get_scale_sizes

    kb = -(-K // 128)
    assert fp8_fp8_get_scale_sizes(M, N, K) == (-(-M // 128) * kb, -(-N // 128) * kb)
    assert fp8_fp8_get_scale_sizes(M, N, K) == R.scale_sizes(M, N, K)


# ---- the oracle's encoder
def test_encoder_maps_every_finite_table_value_to_its_code():
    table = O.fp8_e4m3_table()
    codes = np.array([c for c in range(256) if c & 0x7F != 0x7F], np.uint8)
    np.testing.assert_array_equal(R.e4m3_satfinite_codes(table[codes]), codes)


def test_encoder_rounds_midpoints_to_even():
    table = O.fp8_e4m3_table()
    lo = np.arange(0, 0x7E, dtype=np.uint8)                  # positive codes c, c + 1
    mid = (table[lo].astype(np.float64) + table[lo + 1]) / 2  # 5 significant bits: exact in fp32
    assert np.all(mid.astype(np.float32) == mid)
    want = np.where(lo % 2 == 0, lo, lo + 1).astype(np.uint8)
    np.testing.assert_array_equal(R.e4m3_satfinite_codes(mid.astype(np.float32)), want)
    np.testing.assert_array_equal(R.e4m3_satfinite_codes(-mid.astype(np.float32)), want | 0x80)
    # just off the midpoint goes to the nearer code
    up = np.nextafter(mid.astype(np.float32), np.float32(np.inf))
    np.testing.assert_array_equal(R.e4m3_satfinite_codes(up), lo + 1)


def test_encoder_saturates_finite_and_keeps_nan_and_negative_zero():
    x = np.array([500.0, 1e30, -500.0, 448.0, 464.0, np.inf, -np.inf, -1e30], np.float32)
    np.testing.assert_array_equal(R.e4m3_satfinite_codes(x), [0x7E, 0x7E, 0xFE, 0x7E, 0x7E, 0x7E, 0xFE, 0xFE])
    c = R.e4m3_satfinite_codes(np.array([np.nan, -np.nan, -0.0, 0.0], np.float32))
    assert c[0] & 0x7F == 0x7F and c[1] & 0x7F == 0x7F
    assert c[2] == 0x80 and c[3] == 0x00
    assert np.isnan(O.fp8_e4m3_table()[c[:2]]).all()


def test_oracle_scale_layout_is_mn_major():
    """The oracle's product against a per-block loop written straight from the layout formula."""
    rng = np.random.default_rng(5)
    M, N, K = 200, 272, 300
    a = rng.integers(0, 0x7F, (M, K), dtype=np.uint8)
    b = rng.integers(0, 0x7F, (K, N), dtype=np.uint8)
    sfa, sfb = R.scale_sizes(M, N, K)
    sa = np.exp2(rng.integers(-3, 4, sfa)).astype(np.float32)   # powers of two: every sum is exact in float64
    sb = np.exp2(rng.integers(-3, 4, sfb)).astype(np.float32)
    t = O.fp8_e4m3_table().astype(np.float64)
    MB, NB, KB = -(-M // 128), -(-N // 128), -(-K // 128)
    want = np.zeros((M, N))
    for mb in range(MB):
        for nb in range(NB):
            for kb in range(KB):
                ms, ns, ks = slice(mb * 128, mb * 128 + 128), slice(nb * 128, nb * 128 + 128), slice(kb * 128, kb * 128 + 128)
                want[ms, ns] += float(sa[kb * MB + mb]) * float(sb[kb * NB + nb]) * (t[a[ms, ks]] @ t[b[ks, ns]])
    got = R.gemm_fp8_fp8_nn_f32(a, b, sa, sb)
    np.testing.assert_array_equal(got, want.astype(np.float32))
    np.testing.assert_array_equal(R.gemm_fp8_fp8_nn(a, b, sa, sb), R.e4m3_satfinite_codes(want.astype(np.float32)))
