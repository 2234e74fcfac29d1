"""Rows past 192 in the fused attention + o_proj kernel (attn_oproj_mfma_kernel): a later chunk is staged by live tiles only -
wave w requests tile w, w + 4, w + 8 of the chunk only where the tile's first row is cached - and its counted waits follow
the requests the wave really issued (4 per live tile and image).  Model, oracle rows and bars of test_gpu_attn_fused_trim.py
(Qwen3-0.6B widths, 2 layers, vocabulary 4096, GQA groups 1 / 2 / 4; logits within 1e-2 rel L2 of the oracle, within 6e-3 of
the dot2 kernel, the oracle's token where its margin exceeds 2 % of the largest logit)."""

from __future__ import annotations

import numpy as np
import pytest

from tests import test_gpu_attn_fused_trim as T
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu

pk = pytest.importorskip("pygpukit_amd")
from pygpukit_amd.llm import synthetic as S  # noqa: E402

L = T.L
# first rows of chunk 1 | its tile and owner edges, one live tile per wave at most | 256: second tiles begin | 1, 2 and 3 live tiles per wave
EDGES = (191, 192, 193, 199, 207, 208, 209, 223, 224, 239, 240, 255, 256, 257, 287, 288, 289, 352, 353, 383)


def engine(hkv: int, monkeypatch, max_seq_len: int = T.CACHE, mfma: bool = True, max_batch: int = 1):
    monkeypatch.delenv("PGK_ATTN_MFMA", raising=False)
    if not mfma:
        monkeypatch.setenv("PGK_ATTN_MFMA", "0")
    return S.build_engine_from_weights(T.model_cfg(hkv), T.reference(hkv)[0], max_seq_len=max_seq_len, max_batch=max_batch)


def step_again(eng, tok: int, p: int, replay: bool = False) -> np.ndarray:
    """One more step of token `tok` at position p over the rows already cached."""
    eng.set_state([tok], [p])
    if replay:
        eng.replay(1)
    else:
        eng.decode_step(1)
    eng.synchronize()
    return eng.logits(1).to_numpy()[0].copy()


@pytest.mark.parametrize("hkv", [16, 8, 4])
def test_positions_around_every_live_tile_edge(hkv, monkeypatch):
    _, (toks, _), (want, _) = T.reference(hkv)
    got = {}
    for mode in ("mfma", "dot2"):
        eng = engine(hkv, monkeypatch, mfma=mode == "mfma")
        rows = []
        for p in EDGES:
            rows.append(T.step_at(eng, toks, p))
            assert eng.launches_per_step() == 4 * L + 2, (p, eng.launches_per_step())
        got[mode] = np.stack(rows)
        del eng
    for i, p in enumerate(EDGES):
        assert np.isfinite(got["mfma"][i]).all(), (hkv, p)
        T.check_vs_oracle(got["mfma"][i], want[p], (hkv, p))
        d = rel_err(got["mfma"][i], got["dot2"][i])
        print((hkv, p), "rel err vs dot2", d)
        assert d < 6e-3, (hkv, p, d)


@pytest.mark.parametrize("hkv", [16, 8, 4])
@pytest.mark.parametrize("max_seq_len", [194, 200, 208, 250, 256, 257, 300])
def test_caches_that_clamp_later_chunks(hkv, max_seq_len, monkeypatch):
    """The cache ends inside a live tile of a later chunk: rows past it are requested from its last row and masked.  The logits meet the oracle bars and are, bit for bit, those of an engine whose cache has 512 rows."""
    _, (toks, _), (want, _) = T.reference(hkv)
    short, wide = engine(hkv, monkeypatch, max_seq_len=max_seq_len), engine(hkv, monkeypatch)
    for p in ((192 + max_seq_len) // 2, max_seq_len - 2, max_seq_len - 1):
        got = T.step_at(short, toks, p)
        ref = T.step_at(wide, toks, p)
        assert short.launches_per_step() == 4 * L + 2, (p, short.launches_per_step())
        assert np.isfinite(got).all(), (hkv, max_seq_len, p)
        T.check_vs_oracle(got, want[p], (hkv, max_seq_len, p))
        np.testing.assert_array_equal(got, ref, err_msg=str((hkv, max_seq_len, p)))


@pytest.mark.parametrize("hkv", [16, 8, 4])
def test_the_same_step_repeats_bit_for_bit(hkv, monkeypatch):
    """A read ahead of its DMA would depend on timing: 16 eager runs and 16 replays of the same step from the same state give
    one logits array.  (A tripwire; the proof is the derivation of the wait counts, pinned in test_attn_tail_plan_cpu.py.)"""
    _, (toks, _), (want, _) = T.reference(hkv)
    eng = engine(hkv, monkeypatch)
    for p in (193, 200, 256, 257, 300):
        first = T.step_at(eng, toks, p)
        T.check_vs_oracle(first, want[p], (hkv, p))
        for i in range(15):
            np.testing.assert_array_equal(step_again(eng, toks[p], p), first, err_msg=str((hkv, p, "eager", i)))
        eng.set_state([toks[p]], [p])
        eng.capture(1)
        for i in range(16):
            np.testing.assert_array_equal(step_again(eng, toks[p], p, replay=True), first, err_msg=str((hkv, p, "replay", i)))
        assert eng.launches_per_step() == 4 * L + 2, (p, eng.launches_per_step())


@pytest.mark.parametrize("hkv", [16, 8, 4])
@pytest.mark.parametrize("positions", [(150, 193), (191, 192, 193, 256, 257), (5, 200, 300)])
def test_batch_form_with_and_without_a_second_chunk_in_one_launch(hkv, positions, monkeypatch):
    """OPROJ = false (grid (Hkv, 1, B)): in one launch some workgroups stage one live tile of a second chunk, some several,
    some none."""
    _, streams, wants = T.reference(hkv)
    B = len(positions)
    eng = engine(hkv, monkeypatch, max_batch=B)
    for b, p in enumerate(positions):
        eng.prefill(streams[b % 2][:p], seq=b, want_last_logits=False)
    eng.set_state([streams[b % 2][p] for b, p in enumerate(positions)], list(positions))
    eng.decode_step(B)
    eng.synchronize()
    got = eng.logits(B).to_numpy().copy()
    assert eng.launches_per_step() == 5 * L + 2
    assert any(c["attn"] == "attn_mfma_direct" for c in eng.attn_plan(B, max(positions))), eng.attn_plan(B, max(positions))
    assert np.isfinite(got).all()
    for b, p in enumerate(positions):
        T.check_vs_oracle(got[b], wants[b % 2][p], (hkv, B, b, p))
