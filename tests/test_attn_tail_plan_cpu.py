"""The request plan of the fused MFMA decode attention kernel (csrc/attn_tail_plan.h, the functions attn_oproj_mfma_kernel calls)
pinned through pgk_attn_mfma_plan: for every context of 1..384 cached rows (and some beyond) and every wave, a later chunk costs
the wave four K and four V requests per LIVE tile, and every counted wait allows exactly the requests younger than the ones it
waits for.  Needs no device."""

from __future__ import annotations

import ctypes as C

import pytest

from pygpukit_amd import _hip

CHUNK, WAVES = 192, 4


def plan(c1: int, c0: int, wave: int, pre: int) -> list[int]:
    out = (C.c_int32 * 5)()
    _hip.call("pgk_attn_mfma_plan", c1, c0, wave, pre, out)
    return list(out)


def live_tiles(c0: int, c1: int, wave: int) -> int:
    """Tiles wave, wave + 4, wave + 8 of the chunk at c0 (16 rows each) whose first row is cached."""
    return sum(1 for u in range(3) if c0 + 16 * (wave + WAVES * u) < c1)


@pytest.mark.parametrize("pre", [4, 0])
def test_requests_and_waits_for_every_context_and_wave(pre):
    for c1 in range(1, 385):
        for wave in range(WAVES):
            w_new, w_k0, w_v0, n, w_k = plan(c1, CHUNK, wave, pre)
            tag = (c1, wave, pre)
            # issue phase, in issue (= return) order behind the new token's inputs: the same whatever the context
            order = ["k0"] * 12 + ["v0"] * 12 + ["wo"] * pre
            younger = lambda kind: len(order) - 1 - max(i for i, k in enumerate(order) if k == kind)
            assert w_new == len(order) <= 63, tag                   # vmcnt holds 6 bits
            assert w_k0 == younger("k0"), tag
            assert w_v0 == younger("v0"), tag
            # the second chunk: requests per image = 4 x the wave's live tiles; 4 n K, then 4 n V
            assert n == live_tiles(CHUNK, c1, wave), tag
            assert n == 0 or c1 > CHUNK, tag
            later = ["k"] * (4 * n) + ["v"] * (4 * n)
            assert w_k == len(later) - 4 * n, tag
            # no third chunk up to 384 rows
            assert plan(c1, 2 * CHUNK, wave, pre)[3] == 0, tag


def test_a_third_chunk_stages_its_live_tiles_only():
    for c1 in (385, 400, 401, 447, 448, 449, 512, 575, 576, 600):
        for wave in range(WAVES):
            out = plan(c1, 2 * CHUNK, wave, 4)
            assert out[3] == live_tiles(2 * CHUNK, c1, wave) and out[4] == 4 * out[3], (c1, wave)
            assert plan(c1, CHUNK, wave, 4)[3] == 3, (c1, wave)
