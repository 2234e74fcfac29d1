"""Host tables of the PixArt transformer (reference: src/pygpukit/diffusion/models/dit/embeddings.py).  Both are bit-identical to
the reference's CPU evaluation: float32 positions, float64 products and sin / cos, one rounding to float32.

sinusoidal_embedding is NOT diffusion.ops.sinusoidal_timestep_embedding: it is [sin | cos] (not interleaved) and its frequencies
divide by half_dim - 1.  get_2d_sincos_pos_embed flattens its (h, w) grid column-major (h runs first) although the patch rows it
is added to are row-major - the reference's behaviour, kept as it is."""

from __future__ import annotations

import numpy as np


def sinusoidal_embedding(positions, dim: int) -> np.ndarray:
    pos = np.asarray(positions, dtype=np.float32).reshape(-1).astype(np.float64)
    half = dim // 2
    freqs = np.exp(np.arange(half, dtype=np.float64) * -(np.log(np.float64(10000)) / (half - 1)))
    arg = pos[:, None] * freqs[None, :]
    emb = np.concatenate([np.sin(arg), np.cos(arg)], axis=-1)
    if dim % 2 == 1:
        emb = np.pad(emb, ((0, 0), (0, 1)))
    return emb.astype(np.float32)


def get_2d_sincos_pos_embed(embed_dim: int, grid_size) -> np.ndarray:
    """[grid_h * grid_w, embed_dim] = [height embedding | width embedding], rows in column-major grid order."""
    grid_h, grid_w = (grid_size, grid_size) if isinstance(grid_size, int) else grid_size
    hh, ww = np.meshgrid(np.arange(grid_h, dtype=np.float32), np.arange(grid_w, dtype=np.float32), indexing="ij")
    return np.concatenate([sinusoidal_embedding(hh.flatten("F"), embed_dim // 2),
                           sinusoidal_embedding(ww.flatten("F"), embed_dim // 2)], axis=-1).astype(np.float32)


__all__ = ["sinusoidal_embedding", "get_2d_sincos_pos_embed"]
