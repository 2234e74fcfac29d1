"""Host checks of the integer family: the oracle of tests/int8_ref.py on hand-computed values, the int_gemm_plan leaves at their
boundary shapes, argument errors (raised before anything touches a device) and the export lists."""

from __future__ import annotations

import importlib

import numpy as np
import pytest

from tests import int8_ref as R

F32 = np.float32

NAMES = ("gemm_int8_int32_sm120", "int8_native_gemm_sm120", "gemm_int8_int32_available", "int8_native_gemm_available",
         "gemm_int4_int32_sm120", "gemm_int4_int8_sm120", "int4_gemm_int32_sm120", "int4_gemm_int8_sm120", "gemm_int4_int32_available",
         "int4_gemm_available", "int4_gemv_int32_sm120", "int4_gemv_available", "quantize_to_int8", "dequantize_int8", "linear_int8",
         "matmul_int8_dequant", "int_gemm_plan")
ENTRIES = ("pgk_gemm_int8_nt", "pgk_gemm_int8_dequant_nt", "pgk_gemm_int4_nt", "pgk_gemv_int4", "pgk_quantize_int8_rows",
           "pgk_dequantize_int8_rows", "pgk_linear_int8", "pgk_int_gemm_plan")


def test_names_and_exports():
    import pygpukit_amd as pk
    from pygpukit_amd import _hip, ops
    from pygpukit_amd.ops import quantize
    from pygpukit_amd.ops.matmul import int8 as I

    matmul = importlib.import_module("pygpukit_amd.ops.matmul")      # ops.matmul, the attribute, is the function

    for name in NAMES:
        home = quantize if name in quantize.__all__ else I
        assert getattr(pk, name) is getattr(ops, name) is getattr(home, name) and name in ops.__all__ and name in home.__all__, name
        if home is I:
            assert getattr(matmul, name) is getattr(I, name) and name in matmul.__all__, name
    for mod in (ops, matmul, I, quantize):
        assert len(set(mod.__all__)) == len(mod.__all__)
    assert I.int8_native_gemm_available is I.gemm_int8_int32_available and I.int4_gemm_available is I.gemm_int4_int32_available
    assert I.gemm_int8_int32_available() is True and I.gemm_int4_int32_available() is True and I.int4_gemv_available() is True
    lib = _hip.load()
    for name in ENTRIES:
        assert name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name), name


def test_oracle_on_hand_computed_values():
    v = np.array([[-8, 7, 0, -1, 3, -4]])
    p = R.pack_int4(v)
    assert p.tolist() == [[0x78, 0xF0, 0xC3]] and R.unpack_int4(p).tolist() == v.tolist()
    # rint ties after the division: s = 127 / 127 = 1 -> +-0.5 -> 0, +-2.5 -> +-2, 1.5 -> 2; saturation at 127 and -128
    q, s = R.quantize_rows(np.array([[127, 0.5, -0.5, 2.5, -2.5, 1.5, -0.0], [-200, 200, 199, 0, 0, 0, 0]], F32))
    assert s[0] == F32(1.0) and q[0].tolist() == [127, 0, 0, 2, -2, 2, 0]
    assert q[1].tolist() == [-127, 127, 126, 0, 0, 0, 0]
    q0, s0 = R.quantize_rows(np.zeros((1, 5), F32))              # the 1e-10 floor on an all-zero row
    assert s0[0] == F32(1e-10) and not q0.any()
    qn, sn = R.quantize_rows(np.array([[-4.0, -1.0, -254.0]], F32))   # a row whose maximum is negative
    assert sn[0] == F32(2.0) and qn.tolist() == [[-2, 0, -127]]  # -0.5 ties to even
    # roundf: half away from zero, in the int4 epilogue
    acc = np.array([1, -1, 5, -5, 3], np.int64)
    assert R.scale_round(acc, (0.5, 1.0, 1.0), False).tolist() == [1, -1, 3, -3, 2]
    assert R.scale_round(np.array([127, 128, -128, -129, 1000, -1000]), (1.0, 1.0, 1.0), True).tolist() == [127, 127, -128, -128, 127, -128]
    assert R.scale_round(np.array([2 ** 31 + 5]), (1.0, 1.0, 1.0), False).tolist() == [-(2 ** 31) + 5]   # unit factors: the wrapped integer
    assert R.scale_round(np.array([2 ** 30]), (4.0, 1.0, 1.0), False).tolist() == [2 ** 31 - 1]
    assert R.gemm_int(np.full((1, 3), -128, np.int8), np.full((1, 3), -128, np.int8)).tolist() == [[3 * 16384]]
    assert R.bf16_bits(np.array([1.0, -2.0], F32)).tolist() == [0x3F80, 0xC000]


@pytest.mark.parametrize("op,m,n,k,aligned,leaf", [
    ("gemm_int8", 64, 4096, 128, True, "int8_tile64"), ("gemm_int8", 65, 128, 128, True, "int8_tile64"),
    ("gemm_int8", 2048, 2048, 16, True, "int8_tile128"), ("gemm_int8", 2048, 1920, 16, True, "int8_tile64"),     # 16 x 16 = 256 | 16 x 15
    ("gemm_int8_dequant", 4096, 4096, 24, True, "int8_simple"), ("gemm_int8", 4096, 4096, 16, False, "int8_simple"),
    ("gemm_int4", 4096, 4096, 131040, True, "int4_tile128_planes"), ("gemm_int4", 17, 17, 131104, True, "int4_tile64_ext"),
    ("gemm_int4", 17, 17, 34, True, "int4_simple"), ("gemm_int4", 17, 17, 32, False, "int4_simple"),
    ("gemv_int4", 1, 7, 2048, True, "gemv_int4_stream_r4"), ("gemv_int4", 1, 7, 2080, True, "gemv_int4_stream_r2"),
    ("gemv_int4", 1, 7, 8192, True, "gemv_int4_stream_r2"), ("gemv_int4", 1, 7, 8224, True, "gemv_int4_stream_r1"),
    ("gemv_int4", 1, 7, 4098, True, "gemv_int4_simple"),
    ("linear_int8", 1, 130, 1024, True, "linear_int8_stream_m1"), ("linear_int8", 3, 130, 16, True, "linear_int8_stream_m4"),
    ("linear_int8", 8, 1, 1024, True, "linear_int8_stream_m8"), ("linear_int8", 9, 130, 1024, True, "linear_int8_mfma_64"),
    ("linear_int8", 64, 130, 16, True, "linear_int8_mfma_64"), ("linear_int8", 65, 130, 16, True, "linear_int8_mfma_128"),
    ("linear_int8", 1, 130, 200, True, "linear_int8_simple"), ("linear_int8", 130, 130, 1024, False, "linear_int8_simple"),
])
def test_plan_leaves(op, m, n, k, aligned, leaf):
    from pygpukit_amd.ops import int_gemm_plan

    assert int_gemm_plan(op, m, n, k, aligned) == leaf


def test_plan_rejects():
    from pygpukit_amd.ops import int_gemm_plan

    for bad in (("gemm_int4", 4, 4, 33), ("gemv_int4", 1, 4, 31), ("gemm_fp8", 4, 4, 32), ("gemm_int8", 0, 4, 32)):
        with pytest.raises(ValueError):
            int_gemm_plan(*bad)


def _arr(shape, dtype):
    """An array object that owns no device memory: argument checks run before any device call."""
    from pygpukit_amd.core.array import GPUArray
    from pygpukit_amd.core.dtypes import as_dtype

    return GPUArray(shape, as_dtype(dtype), device_ptr=256, owns_memory=False)


@pytest.mark.parametrize("fn,args,text", [
    ("gemm_int8_int32_sm120", (((4, 16), "uint8"), ((4, 16), "int8"), ((4, 4), "int32")), "gemm_int8_int32_sm120: A must be int8"),
    ("gemm_int8_int32_sm120", (((4, 16), "int8"), ((4, 16), "int8"), ((4, 4), "float32")), "D must be int32"),
    ("int8_native_gemm_sm120", (((4, 16), "int8"), ((4, 32), "int8"), ((4, 4), "int32")), "int8_native_gemm_sm120: K dimension mismatch"),
    ("gemm_int8_int32_sm120", (((4, 16), "int8"), ((5, 16), "int8"), ((4, 4), "int32")), "output shape mismatch"),
    ("gemm_int8_int32_sm120", (((4, 16), "int8"), ((16,), "int8"), ((4, 4), "int32")), "A[M,K], B[N,K], D[M,N] required"),
    ("gemm_int4_int32_sm120", (((4, 16), "int8"), ((4, 16), "uint8"), ((4, 4), "int32")), "A must be uint8 (packed int4)"),
    ("gemm_int4_int8_sm120", (((4, 16), "uint8"), ((4, 16), "uint8"), ((4, 4), "int32")), "gemm_int4_int8_sm120: D must be int8"),
    ("int4_gemm_int32_sm120", (((4, 16), "uint8"), ((4, 8), "uint8"), ((4, 4), "int32")), "int4_gemm_int32_sm120: K dimension mismatch"),
    ("int4_gemv_int32_sm120", (((16,), "uint8"), ((4, 16), "uint8"), ((5,), "int32")), "output shape mismatch"),
    ("int4_gemv_int32_sm120", (((4, 16), "uint8"), ((4, 16), "uint8"), ((4,), "int32")), "A[K/2], B[N,K/2], C[N] required"),
    ("quantize_to_int8", (((4,), "float32"),), "input must be 2D"),
    ("quantize_to_int8", (((4, 4), "int8"),), "input must be Float16"),
    ("dequantize_int8", (((4, 4), "int8"), ((5,), "float16"), "float16"), "scale size must match rows"),
    ("dequantize_int8", (((4, 4), "int8"), ((4,), "float16"), "float32"), "scale dtype must match output dtype"),
    ("linear_int8", (((2, 16), "float32"), ((4, 16), "int8"), ((4,), "float32")), "activation must be Float16 or BFloat16"),
    ("linear_int8", (((2, 16), "float16"), ((4, 32), "int8"), ((4,), "float16")), "weight K dimension mismatch"),
    ("linear_int8", (((2, 16), "float16"), ((4, 16), "int8"), ((4,), "float16"), ((5,), "float16")), "bias size must match N"),
    ("matmul_int8_dequant", (((2, 16), "int8"), ((3,), "float32"), ((4, 16), "int8"), ((4,), "float32")), "a_scale must be float32 [M]"),
    ("matmul_int8_dequant", (((2, 16), "int8"), ((2,), "float32"), ((4, 16), "int8"), ((4,), "float32"), ((4,), "float16")), "bias must be bfloat16"),
])
def test_argument_errors(fn, args, text):
    from pygpukit_amd import ops

    built = [_arr(*a) if isinstance(a, tuple) else a for a in args]
    with pytest.raises(ValueError) as e:
        getattr(ops, fn)(*built)
    assert text in str(e.value)
