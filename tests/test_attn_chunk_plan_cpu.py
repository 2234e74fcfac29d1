"""The chunk length of the fused MFMA decode attention kernel as a compile-time parameter (csrc/attn_tail_plan.h): the request
plan of the 256-row single-pass instantiation through pgk_attn_chunk_plan - for every context of 1..256 cached rows and every
wave - and the host's choice of the chunk per step (am_pick_chunk through pgk_attn_chunk_pick).  The 192-row plan through the
same export must be what pgk_attn_mfma_plan (tests/test_attn_tail_plan_cpu.py) reports.  Needs no device."""

from __future__ import annotations

import ctypes as C

import pytest

from pygpukit_amd import _hip

WAVES = 4


def plan(chunk: int, c1: int, c0: int, wave: int, pre: int) -> list[int]:
    out = (C.c_int32 * 12)()
    _hip.call("pgk_attn_chunk_plan", chunk, c1, c0, wave, pre, out)
    return list(out)


def pick(G: int, rows: int) -> list[int]:
    out = (C.c_int32 * 4)()
    _hip.call("pgk_attn_chunk_pick", G, rows, out)
    return list(out)


@pytest.mark.parametrize("pre", [4, 0])
@pytest.mark.parametrize("chunk", [256, 192])
def test_requests_waits_and_row_masks_for_every_context_and_wave(chunk, pre):
    T = chunk // 64
    for c1 in range(1, 257):
        for wave in range(WAVES):
            out = plan(chunk, c1, 0, wave, pre)
            w_new, w_k0, w_v0, n, w_k, nreq, tiles = out[:7]
            tag = (chunk, c1, wave, pre)
            # issue phase, in issue (= return) order behind the new token's inputs: the whole chunk, whatever the context
            order = ["k0"] * (4 * T) + ["v0"] * (4 * T) + ["wo"] * pre
            younger = lambda kind: len(order) - 1 - max(i for i, k in enumerate(order) if k == kind)
            assert tiles == T and nreq == 4 * T and n == T, tag
            assert w_new == len(order) <= 63, tag                   # vmcnt holds 6 bits
            assert w_k0 == younger("k0") == 4 * T + pre, tag
            assert w_v0 == younger("v0") == pre, tag
            assert w_k == 4 * n, tag
            # rows at or past the context carry weight zero: the mask of every tile the wave owns, at every tile edge
            for u in range(T):
                first = 16 * (wave + WAVES * u)
                want = sum(1 << rl for rl in range(16) if first + rl < c1)
                assert out[7 + u] == want, (tag, u)
            # a later chunk: live tiles only, 4 n K then 4 n V
            later = plan(chunk, c1, chunk, wave, pre)
            live = sum(1 for u in range(T) if chunk + 16 * (wave + WAVES * u) < c1)
            assert later[3] == live and later[4] == 4 * live, tag
            if c1 <= chunk:
                assert later[3] == 0 and not any(later[7:7 + T]), tag       # one pass: nothing of a second chunk


def test_the_192_row_plan_is_the_pinned_one():
    for c1 in (1, 192, 193, 208, 209, 300, 384, 385, 600):
        for c0 in (192, 384):
            for wave in range(WAVES):
                for pre in (4, 0):
                    old = (C.c_int32 * 5)()
                    _hip.call("pgk_attn_mfma_plan", c1, c0, wave, pre, old)
                    assert plan(192, c1, c0, wave, pre)[:5] == list(old), (c1, c0, wave, pre)


def test_a_second_chunk_of_256_rows_stages_live_tiles_only():
    for c1 in (257, 272, 273, 320, 321, 383, 384, 512):
        for wave in range(WAVES):
            out = plan(256, c1, 256, wave, 4)
            live = sum(1 for u in range(4) if 256 + 16 * (wave + WAVES * u) < c1)
            assert out[3] == live and out[4] == 4 * live <= 63, (c1, wave)


def test_bad_arguments_are_refused():
    for args in ((128, 10, 0, 0, 4), (256, 10, 100, 0, 4), (256, 10, 0, 4, 4), (256, 10, 0, 0, 3)):
        with pytest.raises(_hip.PgkError):
            plan(*args)


@pytest.mark.parametrize("G", [1, 2, 4])
def test_host_choice_for_every_row_count(G):
    """One sequence on the fused path: up to 192 rows the 192-row kernel (one pass), 193..256 the 256-row kernel (one pass),
    from 257 on 192-row chunks again (two passes up to SHORT_CTX_B1, then the split path, which has no chunk)."""
    for rows in range(1, 401):
        chunk, lds192, lds256, cu = pick(G, rows)
        assert chunk == (256 if 192 < rows <= 256 else 192), (G, rows)
        assert lds192 < lds256 <= cu == 160 * 1024, (G, lds192, lds256)
        assert lds256 - lds192 == 2 * 64 * 256
        assert 2 * lds192 > cu                               # one workgroup per CU, as today
    assert pick(G, -1)[0] == 192 and pick(G, 0)[0] == 192   # an unknown bound


def test_lds_figures_and_the_fallback():
    # K + V images + the waves' input copies + 5 state records + the normalised heads + q / k / v of the new token
    assert pick(1, 200)[1:3] == [114512, 147280]
    assert pick(2, 200)[1:3] == [117920, 150688]            # 151 KB (decimal) of 160 KiB
    assert pick(4, 200)[1:3] == [128832, 161600]
    # a group whose 256-row form would not fit a CU keeps the 192-row kernel at every row count
    for G in (8, 16):
        assert pick(G, 200)[2] > pick(G, 200)[3]
        assert {pick(G, rows)[0] for rows in range(1, 401)} == {192}, G
