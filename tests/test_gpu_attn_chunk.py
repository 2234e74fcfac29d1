"""The 256-row single-pass instantiation of the fused attention + o_proj kernel (attn_oproj_mfma_kernel<G, true, 256>): one
sequence with 193..256 cached rows stages 16 tiles, 4 per wave, and takes ONE softmax pass where the 192-row kernel takes two.
The host picks the chunk per step (eager: enqueue_step; replay: the short-context sequence captured a second time).

Exact checks run on the stair probes of tests/engine_stair_ref.py through the rig of tests/test_engine_stair_gpu.py (one layer,
head_dim 128, GQA groups 1 / 2 / 4 - the probe's G = 4 shape has one kv head, the others two): attention returns probability
exactly 1.0 there, so the order of the softmax sum does not enter and the stair suite's derived bar holds unchanged.  Random
weights (the model, oracle rows and bars of tests/test_gpu_attn_tail.py: logits within 1e-2 rel L2 of the oracle and the
oracle's token where its margin exceeds 2 % of the largest logit) cover the sum itself."""

from __future__ import annotations

import numpy as np
import pytest

from tests import engine_stair_ref as R
from tests import test_gpu_attn_fused_trim as T
from tests import test_gpu_attn_tail as TT
from tests.test_engine_stair_gpu import Rig

pytestmark = pytest.mark.gpu

pk = pytest.importorskip("pygpukit_amd")

L = T.L
STAIR = [("d128g1", True), ("d128g2", True), ("d128g2", False), ("d128g4", True)]
EDGES = (192, 193, 194, 207, 208, 209, 223, 224, 225, 239, 240, 241, 255, 256, 257)
_RIGS: dict = {}


def chunk_of(p: int) -> int:
    return 256 if 192 < p <= 256 else 192


def rig(shape, qk) -> Rig:
    if (shape, qk) not in _RIGS:
        _RIGS[(shape, qk)] = Rig(shape, qk, R.CACHE_SHORT, 1, ())
    return _RIGS[(shape, qk)]


@pytest.fixture(scope="module", autouse=True)
def _drop_engines():
    yield
    _RIGS.clear()


@pytest.mark.parametrize("shape,qk", STAIR)
def test_context_edges_return_the_last_row(shape, qk):
    """Ascending fill: the winner is row p - 1, the last live row of the last live tile; a row masked too early returns p - 2,
    a clamped or dead row that counts returns a row >= p."""
    r = rig(shape, qk)
    for p in EDGES:
        assert r.plan([p])[0]["attn"] == "attn_oproj_mfma"
        assert r.eng.attn_chunk(1, p) == chunk_of(p), p
        r.step([p], what=("chunk", chunk_of(p)))
        assert r.eng.attn_chunk_state()[0] == chunk_of(p), p
        assert r.eng.launches_per_step() == 4 * 1 + 2


@pytest.mark.parametrize("shape,qk", STAIR)
def test_top_height_in_every_row_group_of_the_fourth_tiles(shape, qk):
    """The top height planted once in every 16-row group of rows 192..255 (the tiles w + 12 of the four waves), at a varying
    offset, and in the first three tiles of a wave: a tile that is dropped, paired with the wrong weights or read from another
    tile's rows loses exactly these."""
    r = rig(shape, qk)
    for g in range(4):
        m = 192 + 16 * g + (7 * g + 3) % 16
        for p in (256, 192 + 16 * g + 16):
            r.step_planted(p, m, what=("fourth tile of wave", g))
            assert r.eng.attn_chunk_state()[0] == 256
        r.step_planted(m + 1, m, what=("last live row of wave", g))
    for m in (0, 70, 135, 191):
        r.step_planted(200, m, what="first three tiles")


@pytest.mark.parametrize("shape,qk", [("d128g2", True), ("d128g4", True)])
def test_stair_eager_and_replayed_steps_agree(shape, qk):
    r = rig(shape, qk)
    for p in (193, 240, 256):
        r.step([p], replay=True, what="replayed")
        assert r.eng.attn_chunk_state()[0] == 256 and r.eng.launches_per_step() == 4 * 1 + 2


@pytest.mark.parametrize("hkv", [16, 8, 4])
def test_random_weights_vs_oracle_and_repeats(hkv, monkeypatch):
    """Contexts 193, 224, 256 against the oracle; then 15 more eager runs and 16 replays of the same step from the same state
    give one logits array (a read ahead of its DMA would depend on timing)."""
    _, (toks, _), (want, _) = T.reference(hkv)
    eng = TT.engine(hkv, monkeypatch)
    for p in (193, 224, 256):
        first = T.step_at(eng, toks, p)
        assert eng.attn_chunk_state()[0] == 256
        assert np.isfinite(first).all()
        T.check_vs_oracle(first, want[p], (hkv, p))
        for i in range(15):
            np.testing.assert_array_equal(TT.step_again(eng, toks[p], p), first, err_msg=str((hkv, p, "eager", i)))
        eng.set_state([toks[p]], [p])
        eng.capture(1)
        for i in range(16):
            np.testing.assert_array_equal(TT.step_again(eng, toks[p], p, replay=True), first, err_msg=str((hkv, p, "replay", i)))
            assert eng.attn_chunk_state()[0] == 256
        assert eng.launches_per_step() == 4 * L + 2


@pytest.mark.parametrize("hkv", [16, 8, 4])
def test_cache_lengths_compute_the_same_bits(hkv, monkeypatch):
    """Requests past the cache end are clamped to its last row and masked: a 208-row, a 256-row and a 512-row cache agree bit
    for bit."""
    _, (toks, _), (want, _) = T.reference(hkv)
    engines = {n: TT.engine(hkv, monkeypatch, max_seq_len=n) for n in (208, 256, 512)}
    for p in (194, 200, 207):
        got = {n: T.step_at(e, toks, p) for n, e in engines.items()}
        for n, e in engines.items():
            assert e.attn_chunk_state()[0] == 256 and e.launches_per_step() == 4 * L + 2
        T.check_vs_oracle(got[512], want[p], (hkv, p))
        np.testing.assert_array_equal(got[208], got[512], err_msg=str((hkv, p, 208)))
        np.testing.assert_array_equal(got[256], got[512], err_msg=str((hkv, p, 256)))


@pytest.mark.parametrize("hkv", [8, 4])
def test_tier_switches_inside_one_replay(hkv, monkeypatch):
    """Positions 188 .. 262: the steps taken eagerly one at a time, replayed one at a time and replayed in ONE call give the same
    tokens (and logits where they can be read) per step; the chunk is 192, then 256 from row 193, then 192 from row 257."""
    _, (toks, _), _ = T.reference(hkv)
    eng = TT.engine(hkv, monkeypatch)
    P0, N = 188, 75

    def start():
        eng.prefill(toks[:P0], want_last_logits=False)
        eng.set_state([toks[P0]], [P0])
        eng.reset_log()
        eng.synchronize()

    def one_by_one(step):
        rows = []
        for i in range(N):
            step()
            eng.synchronize()
            assert eng.attn_chunk_state()[0] == chunk_of(P0 + i) == eng.attn_chunk(1, P0 + i), P0 + i
            assert eng.launches_per_step() == 4 * L + 2
            rows.append(eng.logits(1).to_numpy()[0].copy())
        return np.stack(rows), eng.read_tokens(1, N)[:, 0].copy()

    start()
    eager_logits, eager_tokens = one_by_one(lambda: eng.decode_step(1))
    start()
    eng.capture(1)
    start()
    replay_logits, replay_tokens = one_by_one(lambda: eng.replay(1))
    np.testing.assert_array_equal(replay_tokens, eager_tokens)
    np.testing.assert_array_equal(replay_logits, eager_logits)
    start()
    wide0 = eng.attn_chunk_state()[1]
    eng.replay(N)
    eng.synchronize()
    assert eng.attn_chunk_state() == (192, wide0 + 64)          # rows 193 .. 256 and no other step
    np.testing.assert_array_equal(eng.read_tokens(1, N)[:, 0], eager_tokens)
    np.testing.assert_array_equal(eng.logits(1).to_numpy()[0], eager_logits[-1])


@pytest.mark.parametrize("hkv", [16, 8, 4])
def test_batch_form_stays_on_192_rows(hkv, monkeypatch):
    _, streams, wants = T.reference(hkv)
    positions = (194, 150)
    eng = TT.engine(hkv, monkeypatch, max_batch=2)
    for b, p in enumerate(positions):
        eng.prefill(streams[b][:p], seq=b, want_last_logits=False)
    eng.set_state([streams[b][p] for b, p in enumerate(positions)], list(positions))
    eng.decode_step(2)
    eng.synchronize()
    got = eng.logits(2).to_numpy().copy()
    assert eng.attn_chunk(2, 194) == 192 and eng.attn_chunk_state() == (192, 0)
    assert all(c["attn"] == "attn_mfma_direct" for c in eng.attn_plan(2, 194)), eng.attn_plan(2, 194)
    assert eng.launches_per_step() == 5 * L + 2
    for b, p in enumerate(positions):
        T.check_vs_oracle(got[b], wants[b][p], (hkv, b, p))
