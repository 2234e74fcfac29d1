"""Integer matmuls (reference: native/bindings/gemm/int.cpp - gemm_int8_int32_sm120, gemm_int4_int32_sm120,
gemm_int4_int8_sm120 and their aliases; native/ops/matmul/gemv/int4_int4/sm120 - int4_gemv_int32_sm120).

All of them are NT: A [M, K] times B [N, K] transposed.  int8 operands are int8 arrays; int4 operands are uint8 arrays of
packed signed nibbles, [rows, K/2], k even in the low nibble and k + 1 in the high one, values -8..7.

The accumulator is the exact int32 sum everywhere (v_mfma_i32_16x16x64_i8, v_dot8_i32_i4): where the reference runs int8 on
dp4a and int4 "approximately" through e4m3 and bf16, the results here are the integers themselves, and the int4 scale
epilogue is D = saturate(roundf((float)acc * scale_A * scale_B * descale_D)) in fp32, left to right.  The arithmetic of every
op is restated step by step in tests/int8_ref.py.  Stricter than the reference: int4 needs an even K (the bindings derive
K = 2 * K_packed, so an odd K cannot be expressed through them either)."""

from __future__ import annotations

from pygpukit_amd import _hip
from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import FLOAT_DTYPES, DataType, as_dtype, bfloat16, float32, int8, int32, uint8
from pygpukit_amd.ops._common import call, check_out

INT_GEMM_PLAN_OPS = ("gemm_int8", "gemm_int8_dequant", "gemm_int4", "gemv_int4", "linear_int8")


def int_gemm_plan(op: str, m: int, n: int, k: int, aligned: bool = True) -> str:
    """[build-defined] The kernel a call of the integer family takes, decided on the host (needs no device) by the functions
    the launchers switch on (csrc/int8_plan.h).  `op`: "gemm_int8" / "gemm_int8_dequant" -> int8_tile128 | int8_tile64 |
    int8_simple; "gemm_int4" -> int4_tile{128,64}_{planes,ext} | int4_simple; "gemv_int4" (m ignored) ->
    gemv_int4_stream_r{1,2,4} | gemv_int4_simple; "linear_int8" -> linear_int8_stream_m{1,2,4,8} | linear_int8_mfma_{64,128} |
    linear_int8_simple.  `k` is the unpacked K; `aligned=False`: an operand off 16-byte alignment."""
    lib = _hip.load()
    plan = lib.pgk_int_gemm_plan(str(op).encode(), int(m), int(n), int(k), int(bool(aligned)))
    if plan is None:
        msg = lib.pgk_last_error()
        raise ValueError(msg.decode(errors="replace") if msg else f"int_gemm_plan: invalid call op={op} m={m} n={n} k={k}")
    return plan.decode()


def gemm_int8_int32_available() -> bool:
    """The i8 MFMA GEMM runs on every gfx950 this backend targets (as fp8_available)."""
    return True


def gemm_int4_int32_available() -> bool:
    """The int4 GEMM runs on every gfx950 this backend targets."""
    return True


def int4_gemv_available() -> bool:
    """The int4 GEMV runs on every gfx950 this backend targets."""
    return True


int8_native_gemm_available = gemm_int8_int32_available
int4_gemm_available = gemm_int4_int32_available


def _check_nt(name: str, A: GPUArray, B: GPUArray, D: GPUArray, in_dtype: DataType, in_text: str, out_dtype: DataType, shape_text: str):
    """The checks of the bindings, in their order and with their texts."""
    if A.dtype != in_dtype:
        raise ValueError(f"{name}: A must be {in_text}")
    if B.dtype != in_dtype:
        raise ValueError(f"{name}: B must be {in_text}")
    if D.dtype != out_dtype:
        raise ValueError(f"{name}: D must be {out_dtype.name}")
    if A.ndim != 2 or B.ndim != 2 or D.ndim != 2:
        raise ValueError(f"{name}: {shape_text} required")
    if B.shape[1] != A.shape[1]:
        raise ValueError(f"{name}: K dimension mismatch")
    if D.shape != (A.shape[0], B.shape[0]):
        raise ValueError(f"{name}: output shape mismatch")
    return A.shape[0], B.shape[0], A.shape[1]


def _gemm_int8(name: str, A: GPUArray, B: GPUArray, D: GPUArray) -> None:
    M, N, K = _check_nt(name, A, B, D, int8, "int8", int32, "A[M,K], B[N,K], D[M,N]")
    if M == 0 or N == 0:
        return
    if K == 0:
        D.fill_zeros()
        return
    call("pgk_gemm_int8_nt", A._p, B._p, D._p, M, N, K, None)


def gemm_int8_int32_sm120(A: GPUArray, B: GPUArray, D: GPUArray) -> None:
    """D[M,N] int32 = A[M,K] int8 @ B[N,K]^T int8 (int.cpp:43-74), exact; wraps in two's complement only where the true sum
    leaves int32."""
    _gemm_int8("gemm_int8_int32_sm120", A, B, D)


def int8_native_gemm_sm120(A: GPUArray, B: GPUArray, D: GPUArray) -> None:
    """[Alias for gemm_int8_int32_sm120] (int.cpp:76-107)."""
    _gemm_int8("int8_native_gemm_sm120", A, B, D)


def matmul_int8_dequant(a_q: GPUArray, a_scale: GPUArray, w_q: GPUArray, w_scale: GPUArray, bias: GPUArray | None = None, *,
                        out: GPUArray | None = None, out_dtype: "str | DataType" = bfloat16) -> GPUArray:
    """[build-defined] The W8A8 linear: out[m][n] = (float)(a_q[m] . w_q[n]) * a_scale[m] * w_scale[n] (+ bias[n]) on the
    exact int32 accumulator of gemm_int8_int32_sm120; the products are fp32, left to right, one rounding to `out_dtype`
    (float32 / float16 / bfloat16).  a_q int8 [M,K], w_q int8 [N,K], a_scale float32 [M], w_scale float32 [N], bias [N] in
    the output dtype."""
    name = "matmul_int8_dequant"
    if a_q.dtype != int8 or w_q.dtype != int8:
        raise ValueError(f"{name}: a_q and w_q must be int8")
    if a_q.ndim != 2 or w_q.ndim != 2:
        raise ValueError(f"{name}: a_q[M,K], w_q[N,K] required")
    if a_q.shape[1] != w_q.shape[1]:
        raise ValueError(f"{name}: K dimension mismatch")
    M, K = a_q.shape
    N = w_q.shape[0]
    odt = out.dtype if out is not None else as_dtype(out_dtype)
    if odt not in FLOAT_DTYPES:
        raise ValueError(f"{name}: output dtype must be float32, float16 or bfloat16, got {odt}")
    if a_scale.dtype != float32 or a_scale.shape != (M,):
        raise ValueError(f"{name}: a_scale must be float32 [M] = [{M}], got {a_scale.dtype} {a_scale.shape}")
    if w_scale.dtype != float32 or w_scale.shape != (N,):
        raise ValueError(f"{name}: w_scale must be float32 [N] = [{N}], got {w_scale.dtype} {w_scale.shape}")
    if bias is not None and (bias.dtype != odt or bias.shape != (N,)):
        raise ValueError(f"{name}: bias must be {odt} [N] = [{N}], got {bias.dtype} {bias.shape}")
    c = check_out(out, (M, N), odt, name)
    if M == 0 or N == 0:
        return c
    if K == 0:
        raise ValueError(f"{name}: K must be positive")
    call("pgk_gemm_int8_dequant_nt", a_q._p, a_scale._p, w_q._p, w_scale._p, None if bias is None else bias._p, c._p, M, N, K,
         odt.code, None)
    return c


def _gemm_int4(name: str, A: GPUArray, B: GPUArray, D: GPUArray, out_dtype: DataType, scale_A: float, scale_B: float,
               descale_D: float) -> None:
    M, N, K_packed = _check_nt(name, A, B, D, uint8, "uint8 (packed int4)", out_dtype, "A[M,K/2], B[N,K/2], D[M,N]")
    if M == 0 or N == 0:
        return
    if K_packed == 0:
        D.fill_zeros()
        return
    call("pgk_gemm_int4_nt", A._p, B._p, D._p, M, N, 2 * K_packed, float(scale_A), float(scale_B), float(descale_D),
         int(out_dtype == int8), None)


def gemm_int4_int32_sm120(A: GPUArray, B: GPUArray, D: GPUArray, scale_A: float = 1.0, scale_B: float = 1.0,
                          descale_D: float = 1.0) -> None:
    """D[M,N] int32 = saturate(roundf((A @ B^T) * scale_A * scale_B * descale_D)) on packed int4 operands (int.cpp:121-157);
    with unit factors D is the exact integer product."""
    _gemm_int4("gemm_int4_int32_sm120", A, B, D, int32, scale_A, scale_B, descale_D)


def int4_gemm_int32_sm120(A: GPUArray, B: GPUArray, D: GPUArray, scale_A: float = 1.0, scale_B: float = 1.0,
                          descale_D: float = 1.0) -> None:
    """[Alias for gemm_int4_int32_sm120] (int.cpp:159-195)."""
    _gemm_int4("int4_gemm_int32_sm120", A, B, D, int32, scale_A, scale_B, descale_D)


def gemm_int4_int8_sm120(A: GPUArray, B: GPUArray, D: GPUArray, scale_A: float = 1.0, scale_B: float = 1.0,
                         descale_D: float = 1.0) -> None:
    """As gemm_int4_int32_sm120 with D int8, saturated to -128..127 (int.cpp:198-234)."""
    _gemm_int4("gemm_int4_int8_sm120", A, B, D, int8, scale_A, scale_B, descale_D)


def int4_gemm_int8_sm120(A: GPUArray, B: GPUArray, D: GPUArray, scale_A: float = 1.0, scale_B: float = 1.0,
                         descale_D: float = 1.0) -> None:
    """[Alias for gemm_int4_int8_sm120] (int.cpp:236-272)."""
    _gemm_int4("int4_gemm_int8_sm120", A, B, D, int8, scale_A, scale_B, descale_D)


def int4_gemv_int32_sm120(A: GPUArray, B_nk: GPUArray, C: GPUArray, scale_A: float = 1.0, scale_B: float = 1.0) -> None:
    """C[N] int32 = saturate(roundf((float)(A[K] . B_nk[n]) * scale_A * scale_B)), A uint8 [K/2] and B_nk uint8 [N, K/2] packed
    int4 (int4_gemv.cu:69-82)."""
    name = "int4_gemv_int32_sm120"
    if A.dtype != uint8:
        raise ValueError(f"{name}: A must be uint8 (packed int4)")
    if B_nk.dtype != uint8:
        raise ValueError(f"{name}: B must be uint8 (packed int4)")
    if C.dtype != int32:
        raise ValueError(f"{name}: C must be int32")
    if A.ndim != 1 or B_nk.ndim != 2 or C.ndim != 1:
        raise ValueError(f"{name}: A[K/2], B[N,K/2], C[N] required")
    if B_nk.shape[1] != A.shape[0]:
        raise ValueError(f"{name}: K dimension mismatch")
    if C.shape[0] != B_nk.shape[0]:
        raise ValueError(f"{name}: output shape mismatch")
    N, K_packed = B_nk.shape
    if N == 0:
        return
    if K_packed == 0:
        C.fill_zeros()
        return
    call("pgk_gemv_int4", A._p, B_nk._p, C._p, 2 * K_packed, N, float(scale_A), float(scale_B), None)


__all__ = ["INT_GEMM_PLAN_OPS", "int_gemm_plan", "gemm_int8_int32_available", "int8_native_gemm_available", "gemm_int4_int32_available",
           "int4_gemm_available", "int4_gemv_available", "gemm_int8_int32_sm120", "int8_native_gemm_sm120", "matmul_int8_dequant",
           "gemm_int4_int32_sm120", "int4_gemm_int32_sm120", "gemm_int4_int8_sm120", "int4_gemm_int8_sm120", "int4_gemv_int32_sm120"]
