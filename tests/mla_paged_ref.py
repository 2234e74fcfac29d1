"""Cases and the float64 oracle of batched MLA decode over a paged latent cache: tests/mla_ref.op per sequence over the rows its
block table names.  A case's pages are NaN wherever the kernel must not read: every row at or beyond a sequence's context, every
unreferenced page, and a poison page that every unused table entry points at - so a look-ahead that dereferences too far, or a
missing zero on the value side, shows as NaN in `out`, never as a bad address."""

from __future__ import annotations

import numpy as np

from tests import attn_stair_ref as S
from tests import mla_ref as R

OP_SHAPES = [(1, 1), (1, 20), (1, 128), (2, 16), (5, 20)]          # (q_len, H): tail columns, tiles straddling query rows, four tiles
BLOCK_SIZES = (16, 48, 64)                                          # divides the 32-row tile, straddles tiles, holds two
BOUNDS = (640, 64)                                                  # max_context: several chunks with the merge, one chunk


def contexts(q_len: int, bound: int) -> list[int]:
    """Idle, the query rows alone, either side of a tile, a page multiple at 16 / 48, many tiles; what exceeds the bound IS the bound
    (context_lens <= max_context is the op's contract), which at 64 is again a page multiple and leaves one chunk."""
    return [min(c, bound) for c in (0, q_len, 31, 33, 96, 600)]


def case(q_len: int, heads: int, block_size: int, ctxs, dtype: str):
    """-> q [B, q_len, H, 576] and rows (a list of [ctx_b, 576]) as float64 values of dtype, the pages as uint16 words
    [num_blocks, block_size, 576], block_tables int32 [B, max_blocks].  Physical pages are a random permutation dealt out page index
    by page index across the sequences (shuffled and interleaved); page 0 is the poison page, two more pages belong to nobody."""
    rng = np.random.default_rng(q_len * 100003 + heads * 1009 + block_size * 31 + sum(ctxs) + len(dtype))
    q = S.round_to(rng.standard_normal((len(ctxs), q_len, heads, R.WIDTH)), dtype).astype(np.float64)
    rows = [S.round_to(rng.standard_normal((c, R.WIDTH)), dtype).astype(np.float64) for c in ctxs]
    need = [-(-c // block_size) for c in ctxs]
    num_blocks = 1 + sum(need) + 2
    free = list(1 + rng.permutation(num_blocks - 1))
    pages = np.full((num_blocks, block_size, R.WIDTH), 0x7FC0 if dtype == "bf16" else 0x7E00, np.uint16)
    tables = np.zeros((len(ctxs), max(need) + 2), np.int32)
    for k in range(max(need)):
        for b, c in enumerate(ctxs):
            if k < need[b]:
                tables[b, k] = free.pop()
                n = min(block_size, c - k * block_size)
                pages[tables[b, k], :n] = S.to_words(rows[b][k * block_size:k * block_size + n], dtype)
    return q, rows, pages, tables


def op(q, rows, ctxs, scale: float, rnd=R.same) -> np.ndarray:
    """out [B, q_len, H, 512]: mla_ref.op per sequence; zeros for an idle one."""
    return np.stack([R.op(q[b], rows[b], c, scale, rnd) if c else np.zeros(q.shape[1:3] + (R.LATENT,)) for b, c in enumerate(ctxs)])
