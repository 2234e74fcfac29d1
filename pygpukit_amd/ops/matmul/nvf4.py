"""NVF4: 4-bit e2m1 values with one byte scale per 32 k (reference: src/pygpukit/ops/matmul/nvf4.py, availability
src/pygpukit/ops/matmul/availability.py:85-110; native side native/ops/matmul/gemv/w4a16_bf16/sm120/nvf4_kernels.cu
and native/ops/matmul/gemm/w4a16_bf16/sm120/nvf4_cutlass.cu).

Format: a code c has sign bit 3 and magnitude {0, .5, 1, 1.5, 2, 3, 4, 6}[c & 7]; a byte holds k (even) in its low
nibble and k+1 in its high nibble.  Weights are data uint8 [K/2, N] and scale uint8 [ceil(K/32), N], a scale byte s
being worth (1 + (s&7)/8) * 2^(((s>>3)&15) - 7) (bit 7 ignored).  The arithmetic of every op is restated step by
step in tests/nvf4_ref.py.

Stricter than the reference: K must be even for the quantiser and the GEMV (the reference writes or reads past
the packed data for odd K), buffers must be uint8, the GEMV checks b_data / b_scale against K, and the GEMM needs
K % 32 == 0 (the reference's CUTLASS alignment) and checks `out`."""

from __future__ import annotations

from pygpukit_amd import _hip
from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import bfloat16, uint8
from pygpukit_amd.ops._common import call, check_out, vp


def nvf4_get_sizes(K: int, N: int) -> tuple[int, int]:
    """(data_size, scale_size) in bytes of NVF4 weights for a [K, N] matrix (nvf4.py:15-31)."""
    data_size = (K // 2) * N
    scale_size = ((K + 31) // 32) * N
    return data_size, scale_size


gemv_nvf4_get_sizes = nvf4_get_sizes


def nvf4_nk_get_sizes(N: int, K: int) -> tuple[int, int]:
    """(data_size, scale_size) in bytes of NVF4 weights for an [N, K] matrix in the engine's NK layout: data [N, K/2],
    scale [N, K/32] (K % 32 == 0).  The layout is this project's (the reference has only [K/2, N] / [K/32, N])."""
    return N * (K // 2), N * (K // 32)


def nvf4_bf16_sm120_available() -> bool:
    """The FP4 MFMA GEMM runs on every gfx950 this backend targets (as fp8_available)."""
    return True


def gemv_nvf4_available() -> bool:
    """The NVF4 GEMV and quantiser run on every gfx950 this backend targets (as fp8_available)."""
    return True


gemm_nvf4_bf16_sm120_available = nvf4_bf16_sm120_available
gemv_nvf4_bf16_sm120_available = gemv_nvf4_available


def _flat_size(a: GPUArray) -> int:
    return a.shape[0] * a.shape[1] if a.ndim == 2 else a.size


def quantize_bf16_to_nvf4(input: GPUArray, out_data: GPUArray, out_scale: GPUArray) -> None:
    """Quantise bf16 weights [K, N] into NVF4 data [K/2, N] and scale [ceil(K/32), N] (nvf4.py:34-83): per column
    and 32-row block, scale = max|x| / 6 encoded as a scale byte, codes = nearest e2m1 of x / scale (ties away from
    zero, NaN -> +6)."""
    if input.ndim != 2:
        raise ValueError(f"quantize_bf16_to_nvf4 requires 2D input, got {input.ndim}D")
    if input.dtype != bfloat16:
        raise ValueError(f"quantize_bf16_to_nvf4 requires bfloat16 input, got {input.dtype}")
    K, N = input.shape
    if K % 2:
        raise ValueError(f"quantize_bf16_to_nvf4: K={K} must be even")
    if out_data.dtype != uint8 or out_scale.dtype != uint8:
        raise ValueError(f"quantize_bf16_to_nvf4: out_data / out_scale must be uint8, got {out_data.dtype} / {out_scale.dtype}")
    expected_data_size, expected_scale_size = nvf4_get_sizes(K, N)
    actual_data_size, actual_scale_size = _flat_size(out_data), _flat_size(out_scale)
    if actual_data_size < expected_data_size:
        raise ValueError(f"out_data buffer too small: {actual_data_size} < {expected_data_size}")
    if actual_scale_size < expected_scale_size:
        raise ValueError(f"out_scale buffer too small: {actual_scale_size} < {expected_scale_size}")
    if K == 0 or N == 0:
        return
    call("pgk_quantize_nvf4", input._p, out_data._p, out_scale._p, K, N, None)


def quantize_bf16_to_nvf4_nk(input: GPUArray, out_data: GPUArray, out_scale: GPUArray) -> None:
    """Quantise bf16 weights W [N, K] (PyTorch [out, in]) into the engine's NK layout: data uint8 [N, K/2] (byte j of a
    row holds k = 2j in its low nibble, 2j+1 in its high nibble) and scale uint8 [N, K/32].  The bytes are the transpose
    of quantize_bf16_to_nvf4(W.T)'s, the reference's arithmetic included.  K must be a positive multiple of 32.
    This op is this project's: the reference has no NK layout."""
    if input.ndim != 2:
        raise ValueError(f"quantize_bf16_to_nvf4_nk requires 2D input, got {input.ndim}D")
    if input.dtype != bfloat16:
        raise ValueError(f"quantize_bf16_to_nvf4_nk requires bfloat16 input, got {input.dtype}")
    N, K = input.shape
    if K % 32 or K == 0:
        raise ValueError(f"quantize_bf16_to_nvf4_nk: K={K} must be a positive multiple of 32")
    if out_data.dtype != uint8 or out_scale.dtype != uint8:
        raise ValueError(f"quantize_bf16_to_nvf4_nk: out_data / out_scale must be uint8, got {out_data.dtype} / {out_scale.dtype}")
    expected_data_size, expected_scale_size = nvf4_nk_get_sizes(N, K)
    if _flat_size(out_data) < expected_data_size:
        raise ValueError(f"out_data buffer too small: {_flat_size(out_data)} < {expected_data_size}")
    if _flat_size(out_scale) < expected_scale_size:
        raise ValueError(f"out_scale buffer too small: {_flat_size(out_scale)} < {expected_scale_size}")
    if N == 0:
        return
    call("pgk_quantize_nvf4_nk", input._p, out_data._p, out_scale._p, N, K, None)


def quantize_nvf4_nk(w: GPUArray) -> tuple[GPUArray, GPUArray]:
    """W bf16 [N, K] -> freshly allocated (data uint8 [N, K/2], scale uint8 [N, K/32]) by quantize_bf16_to_nvf4_nk."""
    N, K = w.shape
    data, scale = GPUArray((N, K // 2), uint8), GPUArray((N, K // 32), uint8)
    quantize_bf16_to_nvf4_nk(w, data, scale)
    return data, scale


def gemv_nvf4_bf16(a: GPUArray, b_data: GPUArray, b_scale: GPUArray, *, out: GPUArray | None = None,
                   alpha: float = 1.0) -> GPUArray:
    """C[N] = alpha * A[K] @ B[K, N] with B in NVF4 (nvf4.py:140-198): bf16 in and out, fp32 accumulation in a fixed
    order.  b_data uint8 [K/2, N], b_scale uint8 with at least ceil(K/32) * N bytes; K even, any K % 32."""
    if a.ndim != 1:
        raise ValueError(f"gemv_nvf4_bf16 requires 1D input vector, got {a.ndim}D")
    if a.dtype != bfloat16:
        raise ValueError(f"gemv_nvf4_bf16 requires bfloat16 input, got {a.dtype}")
    if b_data.ndim != 2:
        raise ValueError(f"b_data must be 2D [K/2, N], got {b_data.ndim}D")
    N = b_data.shape[1]
    if out is not None:
        if out.shape != (N,):
            raise ValueError(f"out shape {out.shape} does not match expected ({N},)")
        if out.dtype != bfloat16:
            raise ValueError(f"out dtype {out.dtype} must be bfloat16")
    K = a.shape[0]
    if K % 2 or K == 0:
        raise ValueError(f"gemv_nvf4_bf16: K={K} must be even and positive")
    if b_data.dtype != uint8 or b_data.shape[0] != K // 2:
        raise ValueError(f"gemv_nvf4_bf16: b_data must be uint8 [K/2, N] = [{K // 2}, {N}], got {b_data.dtype} {b_data.shape}")
    scale_size = nvf4_get_sizes(K, N)[1]
    if b_scale.dtype != uint8 or b_scale.size < scale_size:
        raise ValueError(f"gemv_nvf4_bf16: b_scale must be uint8 with at least ceil(K/32)*N = {scale_size} elements, "
                         f"got {b_scale.dtype} {b_scale.shape}")
    c = check_out(out, (N,), bfloat16, "gemv_nvf4_bf16")
    if N == 0:
        return c
    ws_bytes = int(_hip.load().pgk_gemv_nvf4_workspace_bytes(K, N))
    ws = GPUArray((ws_bytes,), uint8) if ws_bytes else None
    call("pgk_gemv_nvf4_bf16", a._p, b_data._p, b_scale._p, c._p, None if ws is None else ws._p, K, N, float(alpha), None)
    return c


gemv_nvf4_bf16_sm120 = gemv_nvf4_bf16


def matmul_nvf4_bf16_sm120(a: GPUArray, b: GPUArray, *, out: GPUArray | None = None) -> GPUArray:
    """D[M, N] = bf16(e2m1(A[M, K]) @ e2m1(B[K, N])) (nvf4.py:86-137): both operands quantised to e2m1 with unit
    scale (thresholds 0.25 .. 5.0, ties away from zero, NaN -> +0, +-inf -> +-6) and multiplied on the FP4 MFMA;
    the fp32 sum of e2m1 products is exact for K < 116000.  K must be a multiple of 32."""
    if a.ndim != 2:
        raise ValueError(f"matmul_nvf4_bf16_sm120 requires 2D arrays, got {a.ndim}D")
    if b.ndim != 2:
        raise ValueError(f"matmul_nvf4_bf16_sm120 requires 2D arrays, got {b.ndim}D")
    if a.shape[1] != b.shape[0]:
        raise ValueError(f"matmul_nvf4_bf16_sm120 dimension mismatch: {a.shape} @ {b.shape}")
    if a.dtype != bfloat16 or b.dtype != bfloat16:
        raise ValueError("matmul_nvf4_bf16_sm120 requires bfloat16 inputs")
    M, K = a.shape
    N = b.shape[1]
    if K % 32 or K == 0:
        raise ValueError(f"matmul_nvf4_bf16_sm120: K={K} must be a positive multiple of 32")
    d = check_out(out, (M, N), bfloat16, "matmul_nvf4_bf16_sm120")
    if M == 0 or N == 0:
        return d
    kp = (K + 127) // 128 * 128
    ws = GPUArray((int(_hip.load().pgk_gemm_nvf4_workspace_bytes(M, N, K)),), uint8)
    b_packed = vp(ws.device_ptr + M * (kp // 2))
    call("pgk_quantize_e2m1_unit", a._p, ws._p, M, K, 0, None)
    call("pgk_quantize_e2m1_unit", b._p, b_packed, N, K, 1, None)
    call("pgk_gemm_fp4_nt", ws._p, b_packed, d._p, M, N, kp, None)
    return d


gemm_nvf4_bf16_sm120 = matmul_nvf4_bf16_sm120

__all__ = ["nvf4_get_sizes", "gemv_nvf4_get_sizes", "quantize_bf16_to_nvf4", "nvf4_nk_get_sizes", "quantize_bf16_to_nvf4_nk",
           "quantize_nvf4_nk", "matmul_nvf4_bf16_sm120", "gemm_nvf4_bf16_sm120",
           "gemv_nvf4_bf16", "gemv_nvf4_bf16_sm120", "nvf4_bf16_sm120_available", "gemm_nvf4_bf16_sm120_available",
           "gemv_nvf4_available", "gemv_nvf4_bf16_sm120_available"]
