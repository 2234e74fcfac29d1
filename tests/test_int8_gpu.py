"""GPU tests of the integer family against tests/int8_ref.py: the integer GEMMs, the int4 GEMV, the quantiser, the dequantiser
and the float32 W8A8 store bit for bit; the 16-bit linears within the project's 16-bit bar (rel_err <= 1e-2 against float64).
Every case asserts the kernel it takes with int_gemm_plan."""

from __future__ import annotations

import numpy as np
import pytest

from tests import int8_ref as R
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu

pk = pytest.importorskip("pygpukit_amd")
from pygpukit_amd import ops  # noqa: E402
from pygpukit_amd.core import from_numpy  # noqa: E402
from pygpukit_amd.core.array import GPUArray  # noqa: E402
from pygpukit_amd.core.dtypes import as_dtype, int8, uint8  # noqa: E402

SENTINEL, PAD = 0x5A, 32     # the byte around every integer output, and the elements of it on either side
# (M, N): a 128-row / 128-column tile short by one and over by one or two, one row, one column; all on 64-row tiles (too few
# workgroups for 256 CUs).  (2049, 2050): 17 x 17 tiles of 128 x 128, one row / two columns into the last ones.
SMALL_MN = [(1, 17), (17, 1), (17, 130), (129, 129), (130, 17), (129, 1), (1, 130)]
BIG_MN = (2049, 2050)


def run_nt(fn, a: np.ndarray, b: np.ndarray, out_dtype, *factors, misalign: bool = False) -> np.ndarray:
    """fn(A, B, D, *factors) with D inside a larger sentinel-filled buffer: returns D and checks that nothing else was written.
    misalign: the operands are views one byte into their buffers."""
    M, N = a.shape[0], b.shape[0]
    if misalign:
        A = from_numpy(np.concatenate([[0], a.ravel()]).astype(a.dtype)).narrow(1, a.size).view(a.shape)
        B = from_numpy(np.concatenate([[0], b.ravel()]).astype(b.dtype)).narrow(1, b.size).view(b.shape)
    else:
        A, B = from_numpy(a), from_numpy(b)
    npdt = out_dtype.to_numpy_dtype()
    big = from_numpy(np.full((M * N + 2 * PAD) * npdt.itemsize, SENTINEL, np.uint8).view(npdt))
    fn(A, B, big.narrow(PAD, M * N).view((M, N)), *factors)
    got = big.to_numpy()
    edge = np.concatenate([got[:PAD], got[PAD + M * N:]])
    assert (edge.view(np.uint8) == SENTINEL).all()
    return got[PAD:PAD + M * N].reshape(M, N)


def int8_operands(M: int, N: int, K: int, seed: int):
    rng = np.random.default_rng(seed)
    a, b = rng.integers(-128, 128, (M, K)).astype(np.int8), rng.integers(-128, 128, (N, K)).astype(np.int8)
    a[M // 2], b[N // 2] = -128, -128          # (-128)^2 occurs in every k of one output
    return a, b


def int4_operands(M: int, N: int, K: int, seed: int):
    rng = np.random.default_rng(seed)
    a, b = rng.integers(-8, 8, (M, K)), rng.integers(-8, 8, (N, K))
    a[0], b[0] = -8, -8
    if M > 1:
        a[1] = 7
    return a, b


# ---- int8 GEMM -------------------------------------------------------------------------------------------------------------------
# K: below one MFMA k, a tail that is no multiple of 64, exactly one tile, two tiles and a tail
@pytest.mark.parametrize("M,N,K,leaf,misalign",
                         [(M, N, K, "int8_tile64", False) for i, (M, N) in enumerate(SMALL_MN) for K in sorted({(16, 80, 128, 272)[i % 4], 272})]
                         + [(*BIG_MN, 80, "int8_tile128", False), (*BIG_MN, 272, "int8_tile128", False),
                            (17, 130, 24, "int8_simple", False), (130, 17, 16, "int8_simple", True), (1, 1, 3, "int8_simple", False)])
def test_gemm_int8_is_exact(M, N, K, leaf, misalign):
    assert ops.int_gemm_plan("gemm_int8", M, N, K, aligned=not misalign) == leaf
    a, b = int8_operands(M, N, K, 1000 * M + N + K)
    got = run_nt(ops.gemm_int8_int32_sm120, a, b, as_dtype("int32"), misalign=misalign)
    np.testing.assert_array_equal(got, R.gemm_int(a, b))


# ---- int4 GEMM -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,leaf",
                         [(M, N, K, "int4_tile64_planes") for i, (M, N) in enumerate(SMALL_MN) for K in sorted({(32, 96, 512, 544)[i % 4], 544})]
                         + [(*BIG_MN, 544, "int4_tile128_planes"), (17, 17, 131104, "int4_tile64_ext"), (17, 130, 34, "int4_simple")])
def test_gemm_int4(M, N, K, leaf):
    assert ops.int_gemm_plan("gemm_int4", M, N, K) == leaf
    a, b = int4_operands(M, N, K, 2000 * M + N + K)
    pa, pb = R.pack_int4(a), R.pack_int4(b)
    acc = R.gemm_int(a, b)
    got = run_nt(ops.gemm_int4_int32_sm120, pa, pb, as_dtype("int32"))
    np.testing.assert_array_equal(got, acc)                                          # unit factors: the integer itself
    if M * N > 10 ** 6:
        return                                                                          # the epilogues are per element: small shapes cover them
    for factors in ((0.5, 0.25, 2.0), (0.3, 1.0, 1.0), (1.0, 0.3, 0.015625)):
        got = run_nt(ops.gemm_int4_int32_sm120, pa, pb, as_dtype("int32"), *factors)
        np.testing.assert_array_equal(got, R.scale_round(acc, factors, False), err_msg=str(factors))
        got8 = run_nt(ops.gemm_int4_int8_sm120, pa, pb, as_dtype("int8"), *factors)
        np.testing.assert_array_equal(got8, R.scale_round(acc, factors, True), err_msg=str(factors))
    want8 = R.scale_round(acc, (1.0, 1.0, 1.0), True)                                   # 64 K and -56 K: both ends saturate
    assert want8[0, 0] == 127 and (M == 1 or want8[1, 0] == -128)
    np.testing.assert_array_equal(run_nt(ops.int4_gemm_int8_sm120, pa, pb, as_dtype("int8")), want8)


# ---- int4 GEMV -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,leaf", [(32, "gemv_int4_stream_r4"), (160, "gemv_int4_stream_r4"), (4096, "gemv_int4_stream_r2"),
                                    (8224, "gemv_int4_stream_r1"), (4098, "gemv_int4_simple")])
@pytest.mark.parametrize("N", [1, 7, 64, 257])
def test_gemv_int4(N, K, leaf):
    assert ops.int_gemm_plan("gemv_int4", 1, N, K) == leaf
    rng = np.random.default_rng(N + K)
    a, b = rng.integers(-8, 8, K), rng.integers(-8, 8, (N, K))
    b[N // 2] = -8
    A, B = from_numpy(R.pack_int4(a)), from_numpy(R.pack_int4(b))
    for sa, sb in ((1.0, 1.0), (0.3, 0.5)):
        big = from_numpy(np.full(N + 2 * PAD, 0x5A5A5A5A, np.int32))
        ops.int4_gemv_int32_sm120(A, B, big.narrow(PAD, N), sa, sb)
        got = big.to_numpy()
        assert (got[:PAD] == 0x5A5A5A5A).all() and (got[PAD + N:] == 0x5A5A5A5A).all()
        np.testing.assert_array_equal(got[PAD:PAD + N], R.gemv_int4(a, b, sa, sb))


# ---- quantiser / dequantiser ---------------------------------------------------------------------------------------------------
TIES = np.array([0.5, -0.5, 2.5, -2.5, 1.5, 3.5], np.float32)


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("cols", [1, 63, 1024, 1031, 4100])      # 4100: past the row-in-registers kernel
@pytest.mark.parametrize("rows", [1, 5])
def test_quantize_to_int8(rows, cols, dtype):
    rng = np.random.default_rng(rows * 10000 + cols)
    x = rng.standard_normal((rows, cols)).astype(np.float32) * np.exp2(rng.integers(-6, 7, (rows, 1))).astype(np.float32)
    if rows > 1:
        x[1] = 0.0                                  # the 1e-10 floor
        x[2] = -np.abs(x[2]) - 1.0                  # the maximum itself is negative
    if cols > TIES.size + 2:
        s = np.float32(0.25)                        # max|x| = 127 s exactly: s is the row's scale and tie * s its exact .5 quotients
        x[-1] = np.clip(x[-1], -31.0, 31.0)
        x[-1, 0], x[-1, 1:1 + TIES.size], x[-1, -1], x[-1, -2] = 127 * s, TIES * s, 0.0, -0.0
    xs = R.to_storage(x, dtype)
    xv = R.from_storage(xs, dtype)
    want_q, want_s = R.quantize_rows(xv)
    if cols > TIES.size + 2:
        assert want_s[-1] == np.float32(0.25) and (xv[-1, 1:1 + TIES.size] / want_s[-1] == TIES).all()   # the ties survive the dtype
        assert want_q[-1, 1:1 + TIES.size].tolist() == [0, 0, 2, -2, 2, 4]
    q, scale = ops.quantize_to_int8(from_numpy(xs))
    assert q.dtype == int8 and q.shape == (rows, cols) and scale.dtype == as_dtype(dtype) and scale.shape == (rows,)
    np.testing.assert_array_equal(q.to_numpy(), want_q)
    assert scale.to_numpy().tobytes() == R.to_storage(want_s, dtype).tobytes()


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_dequantize_int8(dtype):
    rng = np.random.default_rng(7)
    q = rng.integers(-128, 128, (5, 1031)).astype(np.int8)
    ss = R.to_storage(np.exp2(rng.uniform(-8, 4, 5)).astype(np.float32), dtype)
    out = ops.dequantize_int8(from_numpy(q), from_numpy(ss), dtype)
    assert out.dtype == as_dtype(dtype)
    assert out.to_numpy().tobytes() == R.to_storage(R.dequantize_rows(q, R.from_storage(ss, dtype)), dtype).tobytes()


# ---- W8A8 store ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,leaf,dtype,bias", [
    (17, 130, 80, "int8_tile64", "float32", False), (130, 17, 24, "int8_simple", "float32", False), (*BIG_MN, 16, "int8_tile128", "float32", False),
    (129, 130, 272, "int8_tile64", "float16", True), (129, 130, 272, "int8_tile64", "bfloat16", True), (17, 130, 24, "int8_simple", "bfloat16", True),
    (129, 130, 272, "int8_tile64", "float32", True)])
def test_matmul_int8_dequant(M, N, K, leaf, dtype, bias):
    assert ops.int_gemm_plan("gemm_int8_dequant", M, N, K) == leaf
    rng = np.random.default_rng(M + N + K)
    a, w = int8_operands(M, N, K, 5)
    sa, sw = rng.uniform(0.001, 0.02, M).astype(np.float32), rng.uniform(0.001, 0.02, N).astype(np.float32)
    bs = R.to_storage(rng.standard_normal(N).astype(np.float32), dtype) if bias else None
    out = ops.matmul_int8_dequant(from_numpy(a), from_numpy(sa), from_numpy(w), from_numpy(sw), from_numpy(bs) if bias else None, out_dtype=dtype)
    got = R.from_storage(out.to_numpy(), dtype)
    acc = R.gemm_int(a, w)
    if not bias:                                                                        # multiplies only: nothing to contract
        assert dtype == "float32"
        np.testing.assert_array_equal(got, R.dequant_gemm_f32(acc, sa, sw))
    else:
        want = acc.astype(np.float64) * sa.astype(np.float64)[:, None] * sw.astype(np.float64)[None, :] + R.from_storage(bs, dtype).astype(np.float64)
        err = rel_err(got, want)
        print(f"matmul_int8_dequant {M}x{N}x{K} {dtype}: rel_err {err:.3e}")
        assert err <= 1e-2


# ---- weight-only linear ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("K", [16, 200, 1024, 4112])             # 4112: three LDS chunks of the streaming kernel, the last one short
@pytest.mark.parametrize("M,leaf", [(1, "linear_int8_stream_m1"), (8, "linear_int8_stream_m8"), (9, "linear_int8_mfma_64"),
                                    (17, "linear_int8_mfma_64"), (130, "linear_int8_mfma_128")])
def test_linear_int8(M, leaf, K, dtype):
    rng = np.random.default_rng(M * 7 + K)
    for N in (1, 130):
        assert ops.int_gemm_plan("linear_int8", M, N, K) == (leaf if K % 16 == 0 else "linear_int8_simple")
        xs = R.to_storage(rng.standard_normal((M, K)).astype(np.float32), dtype)
        w = rng.integers(-128, 128, (N, K)).astype(np.int8)
        ss = R.to_storage(rng.uniform(0.001, 0.02, N).astype(np.float32), dtype)
        bs = R.to_storage(rng.standard_normal(N).astype(np.float32), dtype)
        base = R.from_storage(xs, dtype).astype(np.float64) @ (w.astype(np.float64) * R.from_storage(ss, dtype).astype(np.float64)[:, None]).T
        for bias in (None, bs):
            out = ops.linear_int8(from_numpy(xs), from_numpy(w), from_numpy(ss), None if bias is None else from_numpy(bias))
            assert out.shape == (M, N) and out.dtype == as_dtype(dtype)
            want = base if bias is None else base + R.from_storage(bs, dtype).astype(np.float64)
            err = rel_err(R.from_storage(out.to_numpy(), dtype), want)
            print(f"linear_int8 M={M} N={N} K={K} {dtype} bias={bias is not None}: rel_err {err:.3e}")
            assert err <= 1e-2
