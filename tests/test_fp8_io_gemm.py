"""GPU tests of the fp8-in / fp8-out GEMMs (matmul_fp8_fp8_sm120, matmul_fp8_fp8_blockwise_sm120 on
pgk_gemm_fp8_fp8_nn) against the restated oracle of tests/fp8_io_ref.py.  Small-integer operands make every fp32
sum exact, so those cases compare codes bit for bit; random operands leave only fp32 summation order."""

from __future__ import annotations

import numpy as np
import pytest

from tests import fp8_io_ref as R

pytestmark = pytest.mark.gpu

pk = pytest.importorskip("pygpukit_amd")
from pygpukit_amd import ops  # noqa: E402
from pygpukit_amd.core import bfloat16, float32, from_numpy  # noqa: E402
from pygpukit_amd.core.array import GPUArray  # noqa: E402
from pygpukit_amd.core.dtypes import uint8  # noqa: E402

CODE = {0: 0x00, 1: 0x38, 2: 0x40, 3: 0x44, 4: 0x48}   # e4m3 codes of small integers; | 0x80 negates


def int_codes(v: np.ndarray) -> np.ndarray:
    c = np.vectorize(lambda x: CODE[abs(int(x))])(v).astype(np.uint8)
    return np.where(v < 0, c | 0x80, c).astype(np.uint8)


def small_int_operands(M, N, K, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(-2, 3, (M, K))
    b = rng.integers(-3, 4, (K, N))
    b[0] = np.arange(N) % 5          # asymmetric: a transposed or mis-mapped B read cannot pass
    b[:, 0] = np.arange(K) % 3 - 1
    return int_codes(a), int_codes(b)


@pytest.mark.parametrize("shape", [(48, 160, 256), (130, 208, 144), (1, 16, 400), (256, 512, 1024), (129, 128, 16)])
def test_unit_scales_bit_exact(shape):
    M, N, K = shape
    a, b = small_int_operands(M, N, K, seed=M + N + K)
    want = R.gemm_fp8_fp8_nn(a, b)
    got = ops.matmul_fp8_fp8_sm120(from_numpy(a), from_numpy(b)).to_numpy()
    assert got.dtype == np.uint8 and got.shape == (M, N)
    np.testing.assert_array_equal(got, want)
    assert np.count_nonzero(want & 0x7F) > want.size // 2      # the test is about values, not zeros


@pytest.mark.parametrize("shape", [(300, 272, 384), (200, 400, 272), (129, 144, 528)])
def test_blockwise_bit_exact(shape):
    """Power-of-two scales that differ per block: exact sums; a transposed (K-major) or per-row reading of either
    scale array changes the result."""
    M, N, K = shape
    a, b = small_int_operands(M, N, K, seed=7 * M + N)
    rng = np.random.default_rng(K)
    sfa, sfb = ops.fp8_fp8_get_scale_sizes(M, N, K)
    sa = np.exp2(rng.integers(-4, 2, sfa)).astype(np.float32)
    sb = np.exp2(rng.integers(-3, 2, sfb)).astype(np.float32)
    want = R.gemm_fp8_fp8_nn(a, b, sa, sb)
    got = ops.matmul_fp8_fp8_blockwise_sm120(from_numpy(a), from_numpy(b), from_numpy(sa), from_numpy(sb)).to_numpy()
    np.testing.assert_array_equal(got, want)
    # the layout matters for these data: K-major readings of the same arrays give other codes
    MB, NB, KB = -(-M // 128), -(-N // 128), -(-K // 128)
    sa_t = sa.reshape(MB, KB).T.reshape(-1)
    sb_t = sb.reshape(NB, KB).T.reshape(-1)
    assert np.count_nonzero(R.gemm_fp8_fp8_nn(a, b, sa_t, sb) != want) > want.size // 10
    assert np.count_nonzero(R.gemm_fp8_fp8_nn(a, b, sa, sb_t) != want) > want.size // 10
    # scales of any shape with the right element count are accepted
    got2 = ops.gemm_fp8_fp8_blockwise_sm120(from_numpy(a), from_numpy(b), from_numpy(sa.reshape(KB, MB)),
                                            from_numpy(sb.reshape(KB, NB))).to_numpy()
    np.testing.assert_array_equal(got2, want)


@pytest.mark.parametrize("shape", [(256, 512, 1024), (1000, 4096, 4096)])
def test_random_blockwise_vs_oracle(shape):
    """Normal operands quantised per 128x128 block; 1/sqrt(K) folded into scale_b keeps the outputs near unit size,
    inside e4m3's range.  fp32 summation order is the only gap: a code may move one e4m3 step next to a rounding
    midpoint, on fewer than 0.1 % of the outputs."""
    M, N, K = shape
    rng = np.random.default_rng(M + K)
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = rng.standard_normal((K, N)).astype(np.float32)
    a, sa = R.quantize_blocks(x)
    bt, sb = R.quantize_blocks(np.ascontiguousarray(w.T), extra=1.0 / np.sqrt(K))
    b = np.ascontiguousarray(bt.T)
    f = R.gemm_fp8_fp8_nn_f32(a, b, sa, sb)
    assert np.mean(np.abs(f) > 448) < 1e-4 and np.std(f) > 0.5
    want = R.e4m3_satfinite_codes(f)
    got = ops.matmul_fp8_fp8_blockwise_sm120(from_numpy(a), from_numpy(b), from_numpy(sa), from_numpy(sb)).to_numpy()
    d = np.abs(R.code_ordinal(got) - R.code_ordinal(want))
    assert d.max() <= 1
    assert np.count_nonzero(d) < 1e-3 * d.size


def test_saturation_and_nan():
    M, N, K = 130, 144, 256
    a = np.full((M, K), 0x58, np.uint8)             # 16.0
    b = np.full((K, N), 0x58, np.uint8)
    b[:, 1::2] = 0xD8                              # -16.0
    got = ops.matmul_fp8_fp8_sm120(from_numpy(a), from_numpy(b)).to_numpy()   # +-65536 per output
    assert np.all(got[:, 0::2] == 0x7E) and np.all(got[:, 1::2] == 0xFE)
    sfa, sfb = ops.fp8_fp8_get_scale_sizes(M, N, K)
    got = ops.matmul_fp8_fp8_blockwise_sm120(from_numpy(a), from_numpy(b), from_numpy(np.full(sfa, 1e10, np.float32)),
                                             from_numpy(np.full(sfb, 1e10, np.float32))).to_numpy()   # ~3e24: finite, far past 448
    assert np.all(got[:, 0::2] == 0x7E) and np.all(got[:, 1::2] == 0xFE)
    # one NaN code in row 3 of A: NaN codes in row 3 of D, nowhere else
    a, b = small_int_operands(M, N, K, seed=3)
    a[3, 200] = 0x7F
    got = ops.matmul_fp8_fp8_sm120(from_numpy(a), from_numpy(b)).to_numpy()
    nan = (got & 0x7F) == 0x7F
    assert nan[3].all() and not np.delete(nan, 3, axis=0).any()
    want = R.gemm_fp8_fp8_nn(a, b)
    np.testing.assert_array_equal(np.delete(got, 3, axis=0), np.delete(want, 3, axis=0))
    assert ((want[3] & 0x7F) == 0x7F).all()


def test_out_is_written_in_place():
    M, N, K = 64, 128, 128
    a, b = small_int_operands(M, N, K, seed=11)
    out = from_numpy(np.full((M, N), 0x11, np.uint8))
    r = ops.matmul_fp8_fp8_sm120(from_numpy(a), from_numpy(b), out=out)
    assert r is out
    np.testing.assert_array_equal(out.to_numpy(), R.gemm_fp8_fp8_nn(a, b))
    sfa, sfb = ops.fp8_fp8_get_scale_sizes(M, N, K)
    out2 = from_numpy(np.full((M, N), 0x11, np.uint8))
    sa, sb = np.full(sfa, 0.5, np.float32), np.full(sfb, 2.0, np.float32)
    assert ops.matmul_fp8_fp8_blockwise_sm120(from_numpy(a), from_numpy(b), from_numpy(sa), from_numpy(sb), out=out2) is out2
    np.testing.assert_array_equal(out2.to_numpy(), R.gemm_fp8_fp8_nn(a, b))


def test_interface_errors_before_launch():
    M, N, K = 32, 48, 64
    a8, b8 = from_numpy(np.zeros((M, K), np.uint8)), from_numpy(np.zeros((K, N), np.uint8))
    sfa, sfb = ops.fp8_fp8_get_scale_sizes(M, N, K)
    sa, sb = from_numpy(np.ones(sfa, np.float32)), from_numpy(np.ones(sfb, np.float32))
    mm, bw = ops.matmul_fp8_fp8_sm120, ops.matmul_fp8_fp8_blockwise_sm120

    def raises(match, fn, *args, **kw):
        with pytest.raises(ValueError, match=match):
            fn(*args, **kw)

    # the reference's own checks, with its messages
    raises(r"matmul_fp8_fp8_sm120 requires 2D arrays, got 1D", mm, from_numpy(np.zeros(K, np.uint8)), b8)
    raises(r"matmul_fp8_fp8_sm120 requires 2D arrays, got 3D", mm, a8, from_numpy(np.zeros((1, K, N), np.uint8)))
    raises(r"matmul_fp8_fp8_sm120 dimension mismatch: \(32, 64\) @ \(48, 48\)", mm, a8, from_numpy(np.zeros((N, N), np.uint8)))
    raises(r"matmul_fp8_fp8_sm120 requires uint8 inputs \(FP8 E4M3\)", mm, a8, from_numpy(np.zeros((K, N), np.float32)))
    raises(r"matmul_fp8_fp8_blockwise_sm120 requires 2D arrays, got 1D", bw, from_numpy(np.zeros(K, np.uint8)), b8, sa, sb)
    raises(r"matmul_fp8_fp8_blockwise_sm120 dimension mismatch", bw, a8, from_numpy(np.zeros((N, N), np.uint8)), sa, sb)
    raises(r"matmul_fp8_fp8_blockwise_sm120 requires uint8 inputs \(FP8\)", bw, from_numpy(np.zeros((M, K), np.float32)),
           b8, sa, sb)
    raises(r"matmul_fp8_fp8_blockwise_sm120 requires float32 scale factors", bw, a8, b8, sa.astype(bfloat16), sb)
    raises(r"matmul_fp8_fp8_blockwise_sm120 requires float32 scale factors", bw, a8, b8, sa, sb.astype(bfloat16))
    # this backend's limits
    raises(r"scale_a / scale_b must hold", bw, a8, b8, from_numpy(np.ones(sfa + 1, np.float32)), sb)
    raises(r"scale_a / scale_b must hold", bw, a8, b8, sa, from_numpy(np.ones((2, sfb), np.float32)))
    raises(r"multiples of 16", mm, a8, from_numpy(np.zeros((K, 40), np.uint8)))
    raises(r"multiples of 16", mm, from_numpy(np.zeros((M, 72), np.uint8)), from_numpy(np.zeros((72, N), np.uint8)))
    raises(r"multiples of 16", bw, from_numpy(np.zeros((M, 72), np.uint8)), from_numpy(np.zeros((72, N), np.uint8)),
           from_numpy(np.ones(1, np.float32)), from_numpy(np.ones(1, np.float32)))
    # out= must be uint8 [M,N]
    raises(r"out dtype", mm, a8, b8, out=GPUArray((M, N), float32))
    raises(r"out shape", mm, a8, b8, out=GPUArray((N, M), uint8))
    raises(r"out shape", bw, a8, b8, sa, sb, out=GPUArray((M, N + 16), uint8))
    # misaligned operand views are refused by the C entry (RuntimeError from the library), never read
    big = from_numpy(np.zeros(M * K + 8, np.uint8))
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        mm(big._view(8, (M, K)), b8)
