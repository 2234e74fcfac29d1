"""The issue phase of the batch-1 fused attention + o_proj kernel (attn_oproj_mfma_kernel): requests from a scalar base and
a 32-bit per-lane offset, wave-owned tiles (wave w requests and reads tiles w, w + 4, w + 8 of a 192-row chunk behind its
own counted waits), the clamp on the byte offsets.  Model and bars of test_gpu_attn_fused_trim.py (Qwen3-0.6B widths,
2 layers, vocabulary 4096, GQA groups 1 / 2 / 4; logits within 1e-2 rel L2 of the oracle, within 6e-3 of the dot2 kernel,
the oracle's token where its margin exceeds 2 % of the largest logit); the oracle rows are that module's, computed once."""

from __future__ import annotations

import numpy as np
import pytest

from tests import test_gpu_attn_fused_trim as T
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu

pk = pytest.importorskip("pygpukit_amd")
from pygpukit_amd.llm import synthetic as S  # noqa: E402

L = T.L
# every 16-row tile boundary at which the owning wave changes, in the first and the second chunk
OWNERSHIP = (0, 1, 15, 16, 17, 31, 32, 47, 48, 63, 64, 65, 79, 80, 127, 128, 129, 175, 176, 177, 191, 192, 193, 207, 208, 209,
             255, 256, 383)


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
def test_ownership_edges_vs_oracle_and_dot2(hkv, monkeypatch):
    _, (toks, _), (want, _) = T.reference(hkv)
    got = {}
    for mode in ("mfma", "dot2"):
        eng = engine(hkv, monkeypatch, mfma=mode == "mfma")
        rows = []
        for p in OWNERSHIP:
            rows.append(T.step_at(eng, toks, p))
            assert eng.launches_per_step() == 4 * L + 2, (p, eng.launches_per_step())
        got[mode] = np.stack(rows)
        del eng
    for i, p in enumerate(OWNERSHIP):
        assert np.isfinite(got["mfma"][i]).all(), (hkv, p)
        T.check_vs_oracle(got["mfma"][i], want[p], (hkv, p))
        d = rel_err(got["mfma"][i], got["dot2"][i])
        print((hkv, p), "rel err vs dot2", d)
        assert d < 6e-3, (hkv, p, d)


@pytest.mark.parametrize("hkv", [16, 8, 4])
@pytest.mark.parametrize("max_seq_len", [130, 192, 200, 208])
def test_short_caches_clamp_and_do_not_change_the_result(hkv, max_seq_len, monkeypatch):
    """Rows past the cache are requested from its last row and masked: the step's logits meet the oracle bars and are, bit
    for bit, those of an engine whose cache has 512 rows."""
    _, (toks, _), (want, _) = T.reference(hkv)
    short, wide = engine(hkv, monkeypatch, max_seq_len=max_seq_len), engine(hkv, monkeypatch)
    for p in (max_seq_len // 2 + 3, max_seq_len - 2, max_seq_len - 1):
        got = T.step_at(short, toks, p)
        ref = T.step_at(wide, toks, p)
        assert np.isfinite(got).all(), (hkv, max_seq_len, p)
        T.check_vs_oracle(got, want[p], (hkv, max_seq_len, p))
        np.testing.assert_array_equal(got, ref, err_msg=str((hkv, max_seq_len, p)))


@pytest.mark.parametrize("hkv", [16, 8, 4])
def test_the_same_step_repeats_bit_for_bit(hkv, monkeypatch):
    """A read ahead of its DMA would depend on timing: 16 eager runs and 16 replays of the same step from the same state
    give one logits array.  (A tripwire; the proof is the derivation of the wait counts in the kernel.)"""
    _, (toks, _), (want, _) = T.reference(hkv)
    eng = engine(hkv, monkeypatch)
    for p in (17, 150, 191, 193, 300):
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
@pytest.mark.parametrize("positions", [(126, 130, 195), (5, 127, 128, 129, 191, 192, 193, 260)])
def test_batch_form_on_both_sides_of_the_staging_edges(hkv, positions, monkeypatch):
    """OPROJ = false (grid (Hkv, 1, B)): every sequence at its own context around rows 128 and 192."""
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
    assert np.isfinite(got).all()
    for b, p in enumerate(positions):
        T.check_vs_oracle(got[b], wants[b % 2][p], (hkv, B, b, p))
