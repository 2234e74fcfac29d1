"""float64 oracle of paged_attention_prefill (NumPy only): per sequence, gather its pages through the block table, then plain
masked softmax attention.  Local row i of a sequence with q_len rows and ctx keys sees key j iff j <= ctx - q_len + i; a row that
sees no key is zeros; rows of the packed batch that no sequence owns stay zero here (the tests compare owned rows only)."""

from __future__ import annotations

import numpy as np


def gather(cache, table_row, ctx: int) -> np.ndarray:
    """cache [num_blocks, Hkv, block_size, D], one sequence's table row -> its first ctx rows as [Hkv, ctx, D]."""
    pos = np.arange(ctx)
    return np.asarray(cache)[table_row[pos // cache.shape[2]], :, pos % cache.shape[2]].transpose(1, 0, 2)


def paged_attention_prefill(q, k_cache, v_cache, block_tables, context_lens, cu_seqlens_q, scale: float = 0.0) -> np.ndarray:
    q = np.asarray(q, np.float64)
    total, hq, d = q.shape
    rep = hq // k_cache.shape[1]
    scale = scale if scale > 0 else 1.0 / np.sqrt(d)
    out = np.zeros_like(q)
    for b, ctx in enumerate(context_lens):
        r0, r1 = int(cu_seqlens_q[b]), int(cu_seqlens_q[b + 1])
        if r1 == r0 or ctx == 0:
            continue
        k = gather(k_cache, block_tables[b], ctx).astype(np.float64)[np.arange(hq) // rep]      # [Hq, ctx, D]
        v = gather(v_cache, block_tables[b], ctx).astype(np.float64)[np.arange(hq) // rep]
        s = np.einsum("ihd,hjd->hij", q[r0:r1], k) * scale
        seen = np.arange(ctx)[None, :] <= ctx - (r1 - r0) + np.arange(r1 - r0)[:, None]
        s = np.where(seen[None], s, -np.inf)
        p = np.where(seen[None], np.exp(s - np.maximum(s.max(axis=-1, keepdims=True), -1e300)), 0.0)
        p /= np.maximum(p.sum(axis=-1, keepdims=True), 1e-300)
        out[r0:r1] = np.einsum("hij,hjd->ihd", p, v)
    return out
