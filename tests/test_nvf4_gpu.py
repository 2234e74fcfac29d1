"""GPU tests of the NVF4 ops (quantize_bf16_to_nvf4, gemv_nvf4_bf16, matmul_nvf4_bf16_sm120) against the restated
oracle of tests/nvf4_ref.py.  The quantisers and the GEMM are compared bit for bit; the GEMV bit for bit on data
whose fp32 sum is exact in any order, and within 1e-2 on random data."""

from __future__ import annotations

import numpy as np
import pytest

from oracle import cpu_ref as O
from tests import nvf4_ref as R
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu

pk = pytest.importorskip("pygpukit_amd")
from pygpukit_amd import ops  # noqa: E402
from pygpukit_amd.core import from_numpy  # noqa: E402
from pygpukit_amd.core.array import GPUArray  # noqa: E402
from pygpukit_amd.core.dtypes import bfloat16, float32, uint8  # noqa: E402

BF16_NAN, BF16_INF, BF16_NINF = 0x7FC0, 0x7F80, 0xFF80


def bits(x: np.ndarray) -> np.ndarray:
    return O.f32_to_bf16_bits(np.ascontiguousarray(x, np.float32))


def weights_bits(K: int, N: int, seed: int) -> np.ndarray:
    """bf16 bits [K, N]: normal values times 2^e with e spread over -20..12 per (32-row block, column); one zero
    block, exact threshold ties under scale 1, NaN and +-inf."""
    rng = np.random.default_rng(seed)
    nsb = (K + 31) // 32
    spread = np.exp2(rng.integers(-20, 13, (nsb, N))).astype(np.float32)
    x = rng.standard_normal((K, N)).astype(np.float32) * np.repeat(spread, 32, axis=0)[:K]
    if K >= 32 and N >= 1:
        below = O.bf16_bits_to_f32(bits(R.THRESH) - 1)          # the bf16 value just below each threshold
        t = np.concatenate([R.THRESH, -R.THRESH, below]).astype(np.float32)
        x[:32, 0] = 0.0
        x[:t.size, 0] = t
        x[t.size, 0] = 6.0                      # scale 1: the ties reach the thresholds exactly
    if N >= 3:
        x[:min(K, 32), 2] = 0.0                 # an all-zero block
    b = bits(x)
    if K >= 64 and N >= 2:
        b[33, 1], b[40, 1], b[41, 1] = BF16_NAN, BF16_INF, BF16_NINF
        b[K - 1, N - 1] = BF16_NAN
    return b


def quantize_dev(b_bits: np.ndarray):
    K, N = b_bits.shape
    ds, ss = ops.nvf4_get_sizes(K, N)
    data = GPUArray((K // 2, N), uint8)
    scale = GPUArray(((K + 31) // 32, N), uint8)
    assert data.size == ds and scale.size == ss
    ops.quantize_bf16_to_nvf4(from_numpy(b_bits), data, scale)
    return data, scale


# ------------------------------------------------------------------------------------------------------ quantiser
@pytest.mark.parametrize("K", [1000, 66, 4096])
@pytest.mark.parametrize("N", [1, 333, 4096])
def test_quantize_bit_exact(K, N):
    b = weights_bits(K, N, seed=K + N)
    data, scale = quantize_dev(b)
    want_d, want_s = R.quantize_nvf4(O.bf16_bits_to_f32(b))
    np.testing.assert_array_equal(scale.to_numpy(), want_s)
    np.testing.assert_array_equal(data.to_numpy(), want_d)
    assert len(np.unique(want_s)) > min(N, 20) // 2      # the scale bytes vary


def test_quantize_flat_buffers():
    """Outputs may be 1-D buffers of at least the sizes nvf4_get_sizes gives (the reference's size-only check)."""
    K, N = 64, 48
    b = weights_bits(K, N, seed=3)
    ds, ss = ops.nvf4_get_sizes(K, N)
    data, scale = GPUArray((ds + 16,), uint8), GPUArray((ss,), uint8)
    ops.quantize_bf16_to_nvf4(from_numpy(b), data, scale)
    want_d, want_s = R.quantize_nvf4(O.bf16_bits_to_f32(b))
    np.testing.assert_array_equal(data.to_numpy()[:ds], want_d.ravel())
    np.testing.assert_array_equal(scale.to_numpy(), want_s.ravel())


# ---------------------------------------------------------------------------------------------------------- GEMV
def exact_operands(K: int, N: int, seed: int):
    """a: small integers; codes random; a quarter of the scale bytes with bit 7 set.  Every fp32 partial sum is
    exact in any order:
      K <= 4096: scales (1 + m/8) * 2^-3 .. 2^-1, any mantissa m: terms are multiples of 2^-7 and
                 sum |term| <= 3*6*0.9375*K < 2^17;
      K >  4096: scales 2^-3 .. 2^1 (mantissa 0): multiples of 2^-4 and sum |term| <= 3*6*2*K < 2^20 (K <= 16384)."""
    rng = np.random.default_rng(seed)
    a = rng.integers(-3, 4, K).astype(np.float32)
    data = rng.integers(0, 256, (K // 2, N)).astype(np.uint8)
    nsb = (K + 31) // 32
    if K <= 4096:
        scale = (rng.integers(4, 7, (nsb, N)) << 3 | rng.integers(0, 8, (nsb, N))).astype(np.uint8)
    else:
        scale = (rng.integers(4, 9, (nsb, N)) << 3).astype(np.uint8)
    scale |= (rng.random((nsb, N)) < 0.25).astype(np.uint8) << 7
    return a, data, scale


@pytest.mark.parametrize("K, N", [(4096, 4096), (1024, 1000), (66, 333), (14336, 256), (2048, 16), (1000, 4096), (1024, 40000)])
@pytest.mark.parametrize("alpha", [1.0, 0.5])
def test_gemv_exact(K, N, alpha):
    a, data, scale = exact_operands(K, N, seed=K * 7 + N)
    want = R.gemv_nvf4(a, data, scale, alpha)
    got = ops.gemv_nvf4_bf16(from_numpy(bits(a)), from_numpy(data), from_numpy(scale), alpha=alpha).to_numpy()
    assert got.shape == (N,)
    np.testing.assert_array_equal(O.bf16_bits_to_f32(got), O.bf16_bits_to_f32(want))
    assert np.count_nonzero(want) > N // 2


@pytest.mark.parametrize("K, N", [(4096, 14336), (14336, 4096), (1000, 333), (130, 4100)])
def test_gemv_random(K, N):
    rng = np.random.default_rng(K + N)
    a = O.bf16_round(rng.standard_normal(K).astype(np.float32))
    data = rng.integers(0, 256, (K // 2, N)).astype(np.uint8)
    scale = rng.integers(0x28, 0x40, ((K + 31) // 32, N)).astype(np.uint8)
    got = ops.gemv_nvf4_bf16(from_numpy(bits(a)), from_numpy(data), from_numpy(scale)).to_numpy()
    assert rel_err(O.bf16_bits_to_f32(got), R.gemv_nvf4_f64(a, data, scale)) <= 1e-2


def test_gemv_out_and_flat_scale():
    K, N = 1000, 333
    a, data, scale = exact_operands(K, N, seed=5)
    out = GPUArray((N,), bfloat16)
    r = ops.gemv_nvf4_bf16(from_numpy(bits(a)), from_numpy(data), from_numpy(np.concatenate([scale.ravel(), np.array([7, 7], np.uint8)])), out=out)
    assert r is out
    np.testing.assert_array_equal(O.bf16_bits_to_f32(out.to_numpy()), O.bf16_bits_to_f32(R.gemv_nvf4(a, data, scale)))


def test_quantize_then_gemv_round_trip():
    K, N = 4096, 1000
    rng = np.random.default_rng(11)
    w = bits(rng.standard_normal((K, N)).astype(np.float32) * 0.02)
    a = O.bf16_round(rng.standard_normal(K).astype(np.float32))
    data, scale = quantize_dev(w)
    got = ops.gemv_nvf4_bf16(from_numpy(bits(a)), data, scale).to_numpy()
    want_d, want_s = R.quantize_nvf4(O.bf16_bits_to_f32(w))
    assert rel_err(O.bf16_bits_to_f32(got), R.gemv_nvf4_f64(a, want_d, want_s)) <= 1e-2
    # and the 4-bit product is a fair estimate of the bf16 one
    assert rel_err(O.bf16_bits_to_f32(got), a.astype(np.float64) @ O.bf16_bits_to_f32(w)) <= 0.2


def test_gemv_graph_replay():
    K, N = 4096, 4096     # the K-split form: a partial-sum workspace and a second kernel in the graph
    a1, data, scale = exact_operands(K, N, seed=21)
    a2 = np.random.default_rng(22).integers(-3, 4, K).astype(np.float32)
    ad, dd, sd = from_numpy(bits(a1)), from_numpy(data), from_numpy(scale)
    out = GPUArray((N,), bfloat16)
    ops.gemv_nvf4_bf16(ad, dd, sd, out=out)          # warm the pool and the kernels outside the capture
    graph = pk.CudaGraph()
    graph.begin_capture()
    ops.gemv_nvf4_bf16(ad, dd, sd, out=out, alpha=0.5)
    graph.end_capture()
    ad.copy_from_numpy(bits(a2))
    graph.replay()
    graph.synchronize()
    np.testing.assert_array_equal(O.bf16_bits_to_f32(out.to_numpy()), O.bf16_bits_to_f32(R.gemv_nvf4(a2, data, scale, 0.5)))


# ---------------------------------------------------------------------------------------------------------- GEMM
def gemm_operands(M, N, K, seed, nan_rows=False):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-7.5, 7.5, (M, K)).astype(np.float32)
    b = rng.uniform(-7.5, 7.5, (K, N)).astype(np.float32)
    b[0] = (np.arange(N) % 13) * 0.5 - 3.0            # asymmetric: a transposed or mis-mapped B read cannot pass
    b[:, 0] = (np.arange(K) % 7) * 0.75 - 2.0
    ab, bb = bits(a), bits(b)
    if nan_rows:
        ab[M // 2] = BF16_NAN
        ab[M - 1, ::3] = BF16_INF
        bb[K // 3, :] = BF16_NAN
        bb[:, N - 1] = BF16_NINF
    return ab, bb


@pytest.mark.parametrize("shape", [(1, 16, 32), (129, 1000, 96), (130, 208, 4096), (256, 512, 1024), (4096, 4096, 4096)])
def test_gemm_bit_exact(shape):
    M, N, K = shape
    ab, bb = gemm_operands(M, N, K, seed=M + N + K)
    codes = R.e2m1_unit(O.bf16_bits_to_f32(bb))
    assert len(np.unique(codes)) == 16 or K * N < 2000   # every code occurs, saturation included
    want = R.gemm_nvf4(O.bf16_bits_to_f32(ab), O.bf16_bits_to_f32(bb))
    got = ops.matmul_nvf4_bf16_sm120(from_numpy(ab), from_numpy(bb)).to_numpy()
    assert got.shape == (M, N) and got.dtype == np.uint16
    np.testing.assert_array_equal(O.bf16_bits_to_f32(got), O.bf16_bits_to_f32(want))
    assert np.count_nonzero(want & 0x7FFF) > want.size // 2


def test_gemm_nan_inf_rows_and_out():
    M, N, K = 70, 200, 160
    ab, bb = gemm_operands(M, N, K, seed=9, nan_rows=True)
    want = R.gemm_nvf4(O.bf16_bits_to_f32(ab), O.bf16_bits_to_f32(bb))
    out = GPUArray((M, N), bfloat16)
    r = ops.gemm_nvf4_bf16_sm120(from_numpy(ab), from_numpy(bb), out=out)
    assert r is out
    got = out.to_numpy()
    assert not np.isnan(O.bf16_bits_to_f32(got)).any()
    np.testing.assert_array_equal(O.bf16_bits_to_f32(got), O.bf16_bits_to_f32(want))


# ---------------------------------------------------------------------------------------------- interface errors
def test_interface_errors():
    bf = lambda *s: GPUArray(s, bfloat16)  # noqa: E731
    u8 = lambda *s: GPUArray(s, uint8)  # noqa: E731
    # quantiser
    with pytest.raises(ValueError, match="2D"):
        ops.quantize_bf16_to_nvf4(bf(64), u8(32), u8(2))
    with pytest.raises(ValueError, match="bfloat16"):
        ops.quantize_bf16_to_nvf4(GPUArray((64, 4), float32), u8(32, 4), u8(2, 4))
    with pytest.raises(ValueError, match="even"):
        ops.quantize_bf16_to_nvf4(bf(63, 4), u8(32, 4), u8(2, 4))
    with pytest.raises(ValueError, match="out_data buffer too small"):
        ops.quantize_bf16_to_nvf4(bf(64, 4), u8(31, 4), u8(2, 4))
    with pytest.raises(ValueError, match="out_scale buffer too small"):
        ops.quantize_bf16_to_nvf4(bf(64, 4), u8(32, 4), u8(7))
    with pytest.raises(ValueError, match="uint8"):
        ops.quantize_bf16_to_nvf4(bf(64, 4), bf(32, 4), u8(2, 4))
    # GEMV
    a, d, s = bf(64), u8(32, 48), u8(2, 48)
    with pytest.raises(ValueError, match="1D"):
        ops.gemv_nvf4_bf16(bf(1, 64), d, s)
    with pytest.raises(ValueError, match="bfloat16"):
        ops.gemv_nvf4_bf16(GPUArray((64,), float32), d, s)
    with pytest.raises(ValueError, match="2D"):
        ops.gemv_nvf4_bf16(a, u8(32 * 48), s)
    with pytest.raises(ValueError, match="out shape"):
        ops.gemv_nvf4_bf16(a, d, s, out=bf(47))
    with pytest.raises(ValueError, match="out dtype"):
        ops.gemv_nvf4_bf16(a, d, s, out=GPUArray((48,), float32))
    with pytest.raises(ValueError, match="even"):
        ops.gemv_nvf4_bf16(bf(63), d, s)
    with pytest.raises(ValueError, match="b_data"):
        ops.gemv_nvf4_bf16(a, u8(31, 48), s)
    with pytest.raises(ValueError, match="b_data"):
        ops.gemv_nvf4_bf16(a, bf(32, 48), s)
    with pytest.raises(ValueError, match="b_scale"):
        ops.gemv_nvf4_bf16(a, d, u8(1, 48))
    with pytest.raises(ValueError, match="b_scale"):
        ops.gemv_nvf4_bf16(a, d, bf(2, 48))
    # GEMM
    with pytest.raises(ValueError, match="2D"):
        ops.matmul_nvf4_bf16_sm120(bf(64), bf(64, 16))
    with pytest.raises(ValueError, match="2D"):
        ops.matmul_nvf4_bf16_sm120(bf(16, 64), bf(64))
    with pytest.raises(ValueError, match="dimension mismatch"):
        ops.matmul_nvf4_bf16_sm120(bf(16, 64), bf(96, 16))
    with pytest.raises(ValueError, match="bfloat16"):
        ops.matmul_nvf4_bf16_sm120(GPUArray((16, 64), float32), bf(64, 16))
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.matmul_nvf4_bf16_sm120(bf(16, 48), bf(48, 16))
    with pytest.raises(ValueError, match="out shape"):
        ops.matmul_nvf4_bf16_sm120(bf(16, 64), bf(64, 16), out=bf(16, 17))
    with pytest.raises(ValueError, match="out dtype"):
        ops.matmul_nvf4_bf16_sm120(bf(16, 64), bf(64, 16), out=GPUArray((16, 16), float32))
