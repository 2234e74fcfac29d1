"""Per-row symmetric int8: quantiser, dequantiser and the weight-only linear (reference: native/bindings/quantize.cpp over
native/ops/quantize/quantize.cu and quantize_kernels.cuh).

The reference's docstrings say "per-column" and "scale: [cols]"; its kernels (and its own argument checks) scale per ROW -
one scale per output channel of a [N, K] weight.  The kernels are the contract here.  bfloat16 is accepted wherever the
reference takes float16, as this project's extension; linear_int8 adds its bias, which the reference checks and then drops."""

from __future__ import annotations

from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import FLOAT_DTYPES, DataType, as_dtype, bfloat16, float16, int8
from pygpukit_amd.ops._common import call


def quantize_to_int8(input: GPUArray) -> tuple[GPUArray, GPUArray]:
    """x [rows, cols] float32 / float16 / bfloat16 -> (q int8 [rows, cols], scale [rows] in the input dtype): per row
    s = max|x| / 127 in fp32 (at least 1e-10), q = clamp(rint(x / s), -128, 127) with ties to even; the quotient uses the
    unrounded fp32 s, the stored scale is s rounded to the input dtype."""
    if input.ndim != 2:
        raise ValueError("quantize_to_int8: input must be 2D [rows, cols]")
    if input.dtype not in FLOAT_DTYPES:
        raise ValueError("quantize_to_int8: input must be Float16, BFloat16 or Float32")
    rows, cols = input.shape
    q, scale = GPUArray((rows, cols), int8), GPUArray((rows,), input.dtype)
    if rows == 0:
        return q, scale
    if cols == 0:
        raise ValueError("quantize_to_int8: cols must be positive")
    call("pgk_quantize_int8_rows", input._p, q._p, scale._p, rows, cols, input.dtype.code, None)
    return q, scale


def dequantize_int8(input: GPUArray, scale: GPUArray, output_dtype: "str | DataType") -> GPUArray:
    """out[r][c] = (float)input[r][c] * (float)scale[r], rounded once to `output_dtype` (float16 / float32 / bfloat16); the
    scale is [rows] in the output dtype."""
    output_dtype = as_dtype(output_dtype)
    if input.dtype != int8:
        raise ValueError("dequantize_int8: input must be Int8")
    if input.ndim != 2:
        raise ValueError("dequantize_int8: input must be 2D [rows, cols]")
    if scale.ndim != 1:
        raise ValueError("dequantize_int8: scale must be 1D [rows]")
    rows, cols = input.shape
    if scale.shape[0] != rows:
        raise ValueError("dequantize_int8: scale size must match rows")
    if output_dtype not in FLOAT_DTYPES:
        raise ValueError("dequantize_int8: output dtype must be Float16, BFloat16 or Float32")
    if scale.dtype != output_dtype:
        raise ValueError("dequantize_int8: scale dtype must match output dtype")
    out = GPUArray((rows, cols), output_dtype)
    if rows and cols:
        call("pgk_dequantize_int8_rows", input._p, scale._p, out._p, rows, cols, output_dtype.code, None)
    return out


def linear_int8(activation: GPUArray, weight_int8: GPUArray, scale: GPUArray, bias: GPUArray | None = None) -> GPUArray:
    """out[M,N] = activation[M,K] @ (weight_int8[N,K] * scale[N])^T (+ bias[N]), fp32 accumulation; activation, scale, bias
    and the result are float16 (as the reference) or bfloat16.  M <= 8 streams the weights once (the decode case), more rows
    run on the MFMA tile loop (int_gemm_plan("linear_int8", ...) names the kernel)."""
    dt = activation.dtype
    if dt not in (float16, bfloat16):
        raise ValueError("linear_int8: activation must be Float16 or BFloat16")
    if weight_int8.dtype != int8:
        raise ValueError("linear_int8: weight must be Int8")
    if scale.dtype != dt:
        raise ValueError(f"linear_int8: scale must be {dt} (the activation dtype)")
    if activation.ndim != 2 or weight_int8.ndim != 2:
        raise ValueError("linear_int8: activation and weight must be 2D")
    M, K = activation.shape
    N = weight_int8.shape[0]
    if weight_int8.shape[1] != K:
        raise ValueError("linear_int8: weight K dimension mismatch")
    if scale.ndim != 1 or scale.shape[0] != N:
        raise ValueError("linear_int8: scale size must match N")
    if bias is not None:
        if bias.dtype != dt:
            raise ValueError(f"linear_int8: bias must be {dt} (the activation dtype)")
        if bias.ndim != 1 or bias.shape[0] != N:
            raise ValueError("linear_int8: bias size must match N")
    out = GPUArray((M, N), dt)
    if M == 0 or N == 0:
        return out
    if K == 0:
        raise ValueError("linear_int8: K must be positive")
    call("pgk_linear_int8", activation._p, weight_int8._p, scale._p, None if bias is None else bias._p, out._p, M, N, K, dt.code, None)
    return out


__all__ = ["quantize_to_int8", "dequantize_int8", "linear_int8"]
