"""Non-causal attention on the reference's 4-D layout (reference: src/pygpukit/diffusion/ops/cross_attention.py): query [B, H, N_q,
D], key / value [B, H, N_kv, D] -> [B, H, N_q, D], N_q and N_kv independent.  One sdpa_noncausal launch per batch element on
views of the inputs; bfloat16 / float16 with head_dim 64 or 128 take the MFMA flash kernel, everything else the fallback.
Attention masks are not implemented: `mask is not None` raises NotImplementedError (the reference applies an additive mask on
its CPU path only)."""

from __future__ import annotations

from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.ops._common import check_out
from pygpukit_amd.ops.nn.attention import sdpa_noncausal


def cross_attention(query: GPUArray, key: GPUArray, value: GPUArray, scale: float = 0.0, mask: GPUArray | None = None, *,
                    out: GPUArray | None = None) -> GPUArray:
    """softmax(Q K^T * scale) V per batch element and head; scale <= 0 -> 1 / sqrt(D)."""
    if mask is not None:
        raise NotImplementedError("cross_attention: attention masks are not implemented (mask must be None)")
    if query.ndim != 4 or key.ndim != 4 or value.ndim != 4:
        raise ValueError("cross_attention expects 4D inputs [B, H, N, D]")
    B, H, n_q, D = query.shape
    if key.shape != value.shape:
        raise ValueError("key and value must have same shape")
    if key.shape[0] != B or key.shape[1] != H or key.shape[3] != D:
        raise ValueError("key/value batch, heads, or head_dim mismatch with query")
    n_kv = key.shape[2]
    o = check_out(out, query.shape, query.dtype, "cross_attention")
    for b in range(B):
        sdpa_noncausal(query._view(b * H * n_q * D, (H, n_q, D)), key._view(b * H * n_kv * D, (H, n_kv, D)),
                       value._view(b * H * n_kv * D, (H, n_kv, D)), scale, out=o._view(b * H * n_q * D, (H, n_q, D)))
    return o


def self_attention(query: GPUArray, key: GPUArray, value: GPUArray, scale: float = 0.0, *, out: GPUArray | None = None) -> GPUArray:
    """cross_attention with Q, K, V from one source."""
    return cross_attention(query, key, value, scale, None, out=out)


__all__ = ["cross_attention", "self_attention"]
