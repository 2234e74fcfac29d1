"""Timestep embeddings (reference: src/pygpukit/diffusion/ops/timestep_embed.py).  The sinusoidal table is host arithmetic and
one upload, bit-identical to the reference's CPU path: float32 timesteps, float64 products and sin / cos, one rounding to
float32; sin in the even columns, cos in the odd ones, frequencies exp(-ln(max_period) * i / half_dim).  (models/dit uses a
different function: [sin | cos] with divisor half_dim - 1.)"""

from __future__ import annotations

import numpy as np

from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import as_dtype
from pygpukit_amd.core.factory import from_numpy


def sinusoidal_timestep_embedding_host(timesteps, embedding_dim: int, max_period: float = 10000.0) -> np.ndarray:
    t = np.asarray(timesteps, dtype=np.float32).reshape(-1).astype(np.float64)
    half = embedding_dim // 2
    freqs = np.exp(-np.log(np.float64(max_period)) * np.arange(half, dtype=np.float64) / half)
    args = t[:, None] * freqs[None, :]
    emb = np.zeros((t.shape[0], embedding_dim), dtype=np.float32)      # an odd embedding_dim keeps a zero last column
    emb[:, 0:2 * half:2] = np.sin(args)
    emb[:, 1:2 * half:2] = np.cos(args)
    return emb


def sinusoidal_timestep_embedding(timesteps, embedding_dim: int, max_period: float = 10000.0, dtype="float32") -> GPUArray:
    """timesteps [B] (GPUArray, ndarray or scalar) -> [B, embedding_dim] in `dtype`."""
    if isinstance(timesteps, GPUArray):
        timesteps = timesteps.astype(as_dtype("float32")).to_numpy()
    return from_numpy(sinusoidal_timestep_embedding_host(timesteps, embedding_dim, max_period)).astype(as_dtype(dtype))


def timestep_mlp(timestep_embedding: GPUArray, fc1_weight: GPUArray, fc1_bias: GPUArray, fc2_weight: GPUArray,
                 fc2_bias: GPUArray) -> GPUArray:
    """Linear -> SiLU -> Linear on [B, D], weights [out, in]: two matmul_nt launches and one activation, all on the device."""
    from pygpukit_amd.ops.matmul import matmul_nt
    from pygpukit_amd.ops.nn.activation import silu

    h = matmul_nt(timestep_embedding, fc1_weight, fc1_bias)
    return matmul_nt(silu(h, out=h), fc2_weight, fc2_bias)


__all__ = ["sinusoidal_timestep_embedding", "timestep_mlp"]
