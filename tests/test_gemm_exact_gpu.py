"""Exact per-element checks of every kernel and tile branch of the dense GEMM family, on the integer operands of
tests/gemm_exact_ref.py: pgk_gemm_nt, pgk_gemm_nn, pgk_w8a16_gemm_nk / _kn, pgk_gemv_fp8_bf16 and pgk_gemm_fp8_nt.

Each case first asserts through gemm_plan that the call takes the kernel the case is there for (the plan is built from the
decision functions the dispatchers switch on), then compares the raw output words with the float64 product, which these
operands make exactly representable (tests/test_gemm_exact_cpu.py proves that, and that a dropped K chunk or tail, shifted
rows, swapped columns, a lost bias, a neighbouring scale block or a transposed tile each change at least one word).  The
output is the first M rows of an (M + 2, N) buffer filled with NaN words: every element must be written, and the two rows
behind it must stay untouched.  There is no whole-tensor bar and no tolerance in this file.
"""

from __future__ import annotations

import numpy as np
import pytest

from tests import gemm_exact_ref as R

pytestmark = pytest.mark.gpu

ENV = ("PGK_GEMM256", "PGK_GEMM256S")
CANARY_ROWS = 2


def _by_op(*ops):
    return [c for c in R.CASES if c.op in ops]


# ---- host <-> device ---------------------------------------------------------------------------------------------------

def _dev(x, dtype, aligned=True):
    """Integer values -> device array of `dtype`; aligned=False: a view that starts one element into a longer buffer."""
    from pygpukit_amd.core import from_numpy

    w = R.to_words(x, dtype)
    w = np.ascontiguousarray(w.view(np.float16) if dtype == "f16" else w)
    if aligned:
        return from_numpy(w)
    flat = np.zeros(w.size + 8, w.dtype)
    flat[1:1 + w.size] = w.ravel()
    a = from_numpy(flat).narrow(1, w.size).view(w.shape)
    assert a.data_ptr() % 16 == w.itemsize
    return a


def _raw(a):
    from pygpukit_amd.core import from_numpy

    return from_numpy(np.ascontiguousarray(a))


def _words(a, dtype) -> np.ndarray:
    """device array -> uint16 words (bf16 / f16) or float32 values."""
    h = a.to_numpy()
    return h if dtype == "f32" or h.dtype == np.uint16 else h.view(np.uint16)


def _nan_buffer(c: R.Case):
    """(M + 2, N) of NaN words and its first M rows as the output view."""
    from pygpukit_amd.core import from_numpy

    shape = (c.m + CANARY_ROWS, c.n)
    if c.dtype == "f32":
        big = from_numpy(np.full(shape, np.nan, np.float32))
    else:
        w = np.full(shape, R.NAN_WORD[c.dtype], np.uint16)
        big = from_numpy(w.view(np.float16) if c.dtype == "f16" else w)
    return big, big.slice_rows(c.m)


def _is_nan_word(w: np.ndarray, dtype: str) -> np.ndarray:
    if dtype == "f32":
        return np.isnan(w)
    exp, frac = (0x7F80, 0x007F) if dtype == "bf16" else (0x7C00, 0x03FF)
    return ((w & exp) == exp) & ((w & frac) != 0)


def _scale_bits(s: np.ndarray) -> np.ndarray:
    return R.to_words(s, "bf16")


def _check(c: R.Case, monkeypatch, run):
    """Plan, call, canaries, words."""
    from pygpukit_amd.ops.matmul import gemm_plan

    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for name, value in c.env:
        monkeypatch.setenv(name, value)
    assert gemm_plan(c.op, c.m, c.n, c.k, R.DTYPE_NAME[c.dtype], c.aligned) == c.leaf
    big, out = _nan_buffer(c)
    assert run(R.make(c), out) is out
    got_all = _words(big, c.dtype)
    got, canary = got_all[:c.m], got_all[c.m:]
    want = R.expected_words(c)
    if c.dtype == "f32":
        assert np.isnan(canary).all(), f"{c}: rows behind the output were written"
    else:
        np.testing.assert_array_equal(canary, R.NAN_WORD[c.dtype], err_msg=f"{c}: rows behind the output were written")
    assert not _is_nan_word(got, c.dtype).any(), f"{c}: {int(_is_nan_word(got, c.dtype).sum())} output words were never written"
    np.testing.assert_array_equal(got, want, err_msg="" if np.array_equal(got, want) else R.explain(c, got, want))


# ---- matmul_nt ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", _by_op("nt"), ids=str)
def test_matmul_nt(case, monkeypatch):
    from pygpukit_amd.ops.matmul import matmul_nt

    def run(o, out):
        return matmul_nt(_dev(o.a, case.dtype, case.aligned), _dev(o.w, case.dtype), _dev(o.bias, case.dtype), out=out)

    _check(case, monkeypatch, run)


# ---- matmul -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", _by_op("nn"), ids=str)
def test_matmul_nn(case, monkeypatch):
    from pygpukit_amd.ops.matmul import matmul

    def run(o, out):
        return matmul(_dev(o.a, case.dtype, case.aligned), _dev(np.ascontiguousarray(o.w.T), case.dtype), out=out)

    _check(case, monkeypatch, run)


# ---- w8a16 --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", _by_op("w8a16_nk"), ids=str)
def test_w8a16_gemm_nk(case, monkeypatch):
    from pygpukit_amd.ops.matmul import w8a16_gemm_nk

    def run(o, out):
        return w8a16_gemm_nk(_dev(o.a, "bf16"), _raw(R.fp8_encode(o.w)), _raw(_scale_bits(o.sw)), out=out)

    _check(case, monkeypatch, run)


@pytest.mark.parametrize("case", _by_op("w8a16_kn"), ids=str)
def test_w8a16_gemm_kn(case, monkeypatch):
    """The [K, N] weight with [K/128, N/128] scales."""
    from pygpukit_amd.ops.matmul import w8a16_gemm

    def run(o, out):
        return w8a16_gemm(_dev(o.a, "bf16"), _raw(R.fp8_encode(o.w).T), _raw(_scale_bits(o.sw).T), out=out)

    _check(case, monkeypatch, run)


# ---- gemv_fp8_bf16 ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", _by_op("gemv_fp8"), ids=str)
def test_gemv_fp8_bf16_batched(case, monkeypatch):
    from pygpukit_amd.ops.matmul import gemv_fp8_bf16_batched

    def run(o, out):
        return gemv_fp8_bf16_batched(_dev(o.a, "bf16"), _raw(R.fp8_encode(o.w)), _raw(_scale_bits(o.sw)), out=out)

    _check(case, monkeypatch, run)


# ---- gemm_fp8_fp8_blockwise_nt ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", _by_op("fp8_nt"), ids=str)
def test_gemm_fp8_fp8_blockwise_nt(case, monkeypatch):
    from pygpukit_amd.ops.matmul import gemm_fp8_fp8_blockwise_nt

    def run(o, out):
        return gemm_fp8_fp8_blockwise_nt(_raw(R.fp8_encode(o.a)), _raw(R.fp8_encode(o.w)), _raw(o.sa.astype(np.float32)),
                                         _raw(_scale_bits(o.sw)), out=out)

    _check(case, monkeypatch, run)


def test_the_forced_fp8_kernels_differ_through_the_plan(monkeypatch):
    """The table runs (256, 256, 256) on both fp8 x fp8 kernels and (300, 520, 384) forced onto the 256-tile one, where it
    falls back: the plan names what really runs."""
    from pygpukit_amd.ops.matmul import gemm_plan

    monkeypatch.delenv("PGK_GEMM256S", raising=False)
    monkeypatch.setenv("PGK_GEMM256", "1")
    assert gemm_plan("fp8_nt", 256, 256, 256, "bfloat16") == "fp8_256" and gemm_plan("fp8_nt", 300, 520, 384, "bfloat16") == "fp8_128"
    monkeypatch.setenv("PGK_GEMM256", "0")
    assert gemm_plan("fp8_nt", 256, 256, 256, "bfloat16") == "fp8_128"
    leaves = {(c.m, c.n, c.k, c.leaf) for c in _by_op("fp8_nt")}
    assert {(256, 256, 256, "fp8_128"), (256, 256, 256, "fp8_256")} <= leaves
