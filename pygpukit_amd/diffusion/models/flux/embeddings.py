"""Host tables of FLUX (reference: src/pygpukit/diffusion/models/flux/embeddings.py): the 3-axis RoPE table, the position ids and
the sinusoidal timestep embedding.  Small float32 NumPy arithmetic, evaluated in the reference's order of operations so that the
results are its float32 values bit for bit; the tables are uploaded once per (ids) and the kernels never evaluate a sine."""

from __future__ import annotations

import numpy as np

F32 = np.float32


def get_1d_rotary_pos_embed(dim: int, pos: np.ndarray, theta: float = 10000.0) -> "tuple[np.ndarray, np.ndarray]":
    """-> (cos, sin), each [len(pos), dim]: angle pos * theta^(-2i / dim) for pair i, each value repeated for both of its pair."""
    exponent = np.arange(0, dim, 2, dtype=F32) / dim
    inv_freq = 1.0 / (theta ** exponent)
    angle = np.outer(pos.astype(F32), inv_freq)
    return np.repeat(np.cos(angle), 2, axis=1), np.repeat(np.sin(angle), 2, axis=1)


def get_rope_frequencies(img_ids: np.ndarray, txt_ids: np.ndarray, axes_dim=(16, 56, 56), theta: float = 10000.0):
    """ids [n, 3] -> (cos, sin) float32 [len(txt) + len(img), sum(axes_dim)]: text rows first; axis a of the ids fills the next
    axes_dim[a] columns."""
    ids = np.concatenate([txt_ids, img_ids], axis=0)
    parts = [get_1d_rotary_pos_embed(d, ids[:, a], theta) for a, d in enumerate(axes_dim)]
    cos = np.concatenate([c for c, _ in parts], axis=1)
    sin = np.concatenate([s for _, s in parts], axis=1)
    return cos.astype(F32), sin.astype(F32)


def apply_rope(x: np.ndarray, cos: np.ndarray, sin: np.ndarray) -> np.ndarray:
    """The host formula on x [B, S, H, D] with tables [S, D]: x * cos + rot * sin, rot[2i] = -x[2i+1], rot[2i+1] = x[2i]."""
    rot = np.empty_like(x)
    rot[..., 0::2] = -x[..., 1::2]
    rot[..., 1::2] = x[..., 0::2]
    return x * cos[None, :, None, :] + rot * sin[None, :, None, :]


def timestep_embedding(timestep: np.ndarray, dim: int = 256, max_period: float = 10000.0) -> np.ndarray:
    """[B] -> [B, dim] float32: [cos | sin] of timestep * exp(-ln(max_period) * i / half), a zero column when dim is odd.  The
    frequencies and the products are float64 (as the reference's expression evaluates: its logarithm is a float64 scalar), the
    timestep is rounded to float32 first and the result once."""
    half = dim // 2
    freqs = np.exp(-np.log(np.float64(max_period)) * np.arange(0, half, dtype=F32).astype(np.float64) / half)
    args = np.asarray(timestep)[:, None].astype(F32).astype(np.float64) * freqs[None, :]
    emb = np.concatenate([np.cos(args), np.sin(args)], axis=-1)
    if dim % 2 == 1:
        emb = np.concatenate([emb, np.zeros_like(emb[:, :1])], axis=-1)
    return emb.astype(F32)


def prepare_image_ids(batch_size: int, height: int, width: int, patch_size: int = 1) -> np.ndarray:
    """[B, h * w, 3] float32 rows (0, row, col) in row-major order."""
    h, w = height // patch_size, width // patch_size
    rows, cols = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    ids = np.stack([np.zeros(h * w, dtype=rows.dtype), rows.reshape(-1), cols.reshape(-1)], axis=-1)
    return np.tile(ids[None], (batch_size, 1, 1)).astype(F32)


def prepare_text_ids(batch_size: int, seq_len: int) -> np.ndarray:
    """[B, seq_len, 3] float32 rows (index, 0, 0)."""
    ids = np.zeros((seq_len, 3), F32)
    ids[:, 0] = np.arange(seq_len)
    return np.tile(ids[None], (batch_size, 1, 1))


__all__ = [
    "get_1d_rotary_pos_embed",
    "get_rope_frequencies",
    "apply_rope",
    "timestep_embedding",
    "prepare_image_ids",
    "prepare_text_ids",
]
