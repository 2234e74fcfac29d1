"""Exact visible-key checks of the native engine's own attention code, on every decode and prefill path.

The probe models of tests/engine_stair_ref.py make the fp32 logits of a step read out WHICH cache row attention returned:
logits[:H] = rmsnorm(embedding + V row of the highest visible height).  Heights are placed by choosing token sequences -
nothing is written into the cache behind the engine's back:

  * every slot's whole cache is prefilled with ascending heights (row j: height j + 1), then a height-0 token is decoded at
    position p.  The winner is row p - 1; a lost tail key returns row p - 2, a visible stale key a row >= p + 1, a wrong
    slot or kv head another tag's or head's row;
  * a one-token prefill plants the top height at row m (and puts the old token back afterwards): the winner is row m, so a
    key lost in the MIDDLE of the context - a dropped tile, trip or split-KV slice - shows as well.

Every logit is compared with the float64 readout of the V row AS READ BACK from the engine's cache (Engine.kv_cache), inside
a bar derived from the rounding points (engine_stair_ref.logit_bar: fp32 RMSNorm over H terms and the fp32 store, plus one
bf16 rounding where the path's lm_head reads bf16 activations).  Nothing is allowed for attention or o_proj.  The cache is
checked on its own: K stair columns bit for bit, V rows inside v_bar, for the rows of every prefill and decode step.
Which kernel ran is asserted through Engine.attn_plan (the launcher's own decision functions) and the launch count.
No whole-tensor tolerance anywhere.  NVF4 is out of scope (heights are not representable).  fp8 (w8a16) engines get their
weights as e4m3 codes under power-of-two block scales encoded by the probe itself (engine_stair_ref.encode_e4m3_blocks), not
by the project's quantiser: stair, identity and copies are exact and the GEMV and MFMA paths see one matrix."""

from __future__ import annotations

import os

import numpy as np
import pytest

from oracle import cpu_ref as O
from tests import engine_stair_ref as R

pytestmark = pytest.mark.gpu

pk = pytest.importorskip("pygpukit_amd")
from pygpukit_amd.core.dtypes import bfloat16  # noqa: E402
from pygpukit_amd.core.factory import from_numpy, zeros  # noqa: E402
from pygpukit_amd.llm import synthetic as S  # noqa: E402
from pygpukit_amd.llm.engine import Engine  # noqa: E402

F32, F64 = np.float32, np.float64
SWITCHES = ("PGK_FUSED_ATTN", "PGK_ATTN_MFMA", "PGK_MERGED_OPROJ", "PGK_BATCHED_MFMA", "PGK_BATCHED_MAX", "PGK_PACKED_PREFILL",
            "PGK_PACKED_DECODE", "PGK_PACKED_RESID", "PGK_PACKED_LMHEAD")


class Rig:
    """One engine on a probe model with every slot's cache holding the ascending fill (slot s carries tag s % 4)."""

    def __init__(self, shape, qk, cache, max_batch, env, fp8=False):
        self.p = p = R.probe(shape, qk, fp8)
        self.cache, self.B = cache, max_batch
        saved = {k: os.environ.pop(k, None) for k in SWITCHES}
        try:
            os.environ.update(dict(env))
            w = p.weights
            layers = [S.engine_layer_arrays(lw, "bf16") for lw in w["layers"]]
            if fp8:         # the probe's own codes and power-of-two block scales (bf16 words), as the engine stores them
                for name, (codes, sbits) in p.fp8.items():
                    layers[0][name], layers[0]["s" + name[1:]] = from_numpy(codes), from_numpy(sbits)
            self.eng = Engine(p.cfg, S._bf16(w["embed"]), layers, S._bf16(w["final_norm"]), S._bf16(w["lm_head"]), max_seq_len=cache,
                              max_batch=max_batch, weight_format="fp8" if fp8 else "bf16", use_qk_norm=qk)
        finally:
            for k in SWITCHES:
                os.environ.pop(k, None)
                if saved[k] is not None:
                    os.environ[k] = saved[k]
        self.fill = [R.fill_tokens(cache, s % R.NTAGS) for s in range(R.NTAGS)]
        for s in range(max_batch):
            self.eng.prefill(self.fill[s % R.NTAGS], seq=s, want_last_logits=False)
        self.eng.synchronize()
        for s in range(max_batch):
            self.check_cache_rows(s, 0, self.fill[s % R.NTAGS], "fill")
        self.captured = 0

    # ---- cache access
    def cache_words(self):
        k, v = self.eng.kv_cache(0)
        return k.to_numpy(), v.to_numpy()          # uint16 [B, Hkv, cache, D]: the whole cache (explain() only)

    def rows_words(self, s: int, r0: int, n: int):
        """K and V words of rows r0 .. r0 + n - 1 of slot s: uint16 [Hkv, n, D] each - only these rows are copied."""
        p = self.p
        out = []
        for c in self.eng.kv_cache(0):
            out.append(np.stack([c._view(((s * p.Hkv + h) * self.cache + r0) * p.D, (n, p.D)).to_numpy() for h in range(p.Hkv)]))
        return out

    def v_row(self, s: int, r: int) -> np.ndarray:
        """V cache row r of slot s: float32 [Hkv, D]."""
        p = self.p
        _, v = self.eng.kv_cache(0)
        return np.stack([O.bf16_bits_to_f32(v._view(((s * p.Hkv + h) * self.cache + r) * p.D, (p.D,)).to_numpy()) for h in range(p.Hkv)])

    def check_cache_rows(self, s: int, r0: int, toks, what) -> None:
        """Rows r0 .. of slot s hold `toks`: K stair columns bit for bit (a set bit or complement: kappa's bf16 word; a cleared
        one: the partner's kappa * sin(angle), below k_zero_bound), V inside v_bar of the float64 W_v . rmsnorm(x)."""
        p = self.p
        kw, vw = self.rows_words(s, r0, len(toks))
        cols = np.concatenate([p.bit_cols, p.cmp_cols])
        bits = p.k_expected_bits(toks)                                      # [n, 24]
        v64 = p.v_rows(toks)                                                # [n, Hkv, D]
        for h in range(p.Hkv):
            k = kw[h][:, cols]
            wrong = (k != p.k_bit_word()) & (bits == 1)
            assert not wrong.any(), f"{what}: slot {s} kv head {h}: K stair word wrong at (row, column) {np.argwhere(wrong)[:4] + [r0, 0]}"
            zero = np.abs(O.bf16_bits_to_f32(k)[bits == 0])
            assert (zero <= p.k_zero_bound(self.cache)).all(), f"{what}: slot {s} kv head {h}: a cleared K stair column holds {zero.max()}"
            v = O.bf16_bits_to_f32(vw[h]).astype(F64)
            over = np.abs(v - v64[:, h]) > p.v_bar(v64)[:, h]
            assert not over.any(), f"{what}: slot {s} kv head {h}: V outside its bar at (row, element) {np.argwhere(over)[:4] + [r0, 0]}"

    # ---- comparing logits
    def explain(self, s: int, tok: int, got: np.ndarray) -> str:
        p = self.p
        _, vw = self.cache_words()
        vc = O.bf16_bits_to_f32(vw)
        out = []
        for h in range(p.Hkv):
            slot, kvh, row, d = R.nearest_row(p, tok, got[:p.H], vc, h)
            out.append(f"query heads of kv head {h} return the V row nearest to slot {slot} kv head {kvh} row {row} (distance {d:.2e})")
        return "; ".join(out)

    def compare(self, s: int, tok: int, got: np.ndarray, row: int, n_bf16: int, what) -> None:
        """got [V] against the readout of cache row `row` of slot s."""
        p = self.p
        want = p.logits_from_v(tok, self.v_row(s, row))
        ok = np.isfinite(got).all() and (np.abs(got[:p.H].astype(F64) - want) <= p.logit_bar(want, n_bf16)).all() and not got[p.H:].any()
        if not ok:
            worst = float((np.abs(got[:p.H].astype(F64) - want) / p.logit_bar(want, n_bf16)).max())
            raise AssertionError(f"{what}: slot {s} expected cache row {row}; worst element {worst:.3g} x the bar, "
                                 f"logits beyond H nonzero: {bool(got[p.H:].any())}; {self.explain(s, tok, got)}")

    # ---- one decode step
    def plan(self, positions):
        return self.eng.attn_plan(len(positions), max(positions))

    def step(self, positions, *, replay=False, planted=None, what="", check_new_row=True) -> None:
        """Height-0 tokens at `positions` (one per slot), one step, every slot's logits against its winner - row p - 1 (p = 0:
        the token's own row), or `planted` = {slot: row} - then the new rows are checked and the fill put back."""
        p, eng, B = self.p, self.eng, len(positions)
        toks = [int(R.token(0, s % R.NTAGS)) for s in range(B)]
        n16 = {}
        for ch in self.plan(positions):
            for s in range(ch["b0"], ch["b0"] + ch["m"]):
                n16[s] = 0 if (ch["form"] == "gemv" and ch["m"] <= 2) else 1    # fp32 activations into the lm_head GEMV of 1 / 2 sequences only
        eng.set_state(toks, list(positions))
        if replay:
            if self.captured != B:
                eng.capture(B)
                eng.set_state(toks, list(positions))
                self.captured = B
            eng.replay(1)
        else:
            eng.decode_step(B)
        eng.synchronize()
        got = eng.logits(B).to_numpy().copy()
        try:
            for s, pos in enumerate(positions):
                row = (planted or {}).get(s, pos - 1 if pos else 0)
                self.compare(s, toks[s], got[s], row, n16[s], (what, "positions", tuple(positions)))
            if check_new_row:
                for s, pos in enumerate(positions):
                    self.check_cache_rows(s, pos, [toks[s]], (what, "the step's own row", pos))
        finally:        # a failing comparison must not leave height-0 rows in a rig that later tests share
            for s, pos in enumerate(positions):
                eng.prefill([self.fill[s % R.NTAGS][pos]], seq=s, start_pos=pos, want_last_logits=False)

    def step_planted(self, pos: int, m: int, what="", **kw) -> None:
        """Slot 0 only: the top height at row m < pos by a one-token prefill, the step, the old token back."""
        assert m < pos <= 4094
        self.eng.prefill([int(R.token(R.TOP, 0))], seq=0, start_pos=m, want_last_logits=False)
        try:
            self.step([pos], planted={0: m}, what=(what, "top height planted at row", m), check_new_row=False, **kw)
        finally:
            self.eng.prefill([self.fill[0][m]], seq=0, start_pos=m, want_last_logits=False)


_RIGS: dict = {}


def rig(shape, qk=True, cache=R.CACHE_SHORT, max_batch=1, env=(), fp8=False) -> Rig:
    """Engines are built once per (shape, family, cache, batch, switches, weight format) per module."""
    key = (shape, qk, cache, max_batch, tuple(env), fp8)
    if key not in _RIGS:
        _RIGS[key] = Rig(shape, qk, cache, max_batch, env, fp8)
    return _RIGS[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_engines():
    yield
    _RIGS.clear()


def assert_plan(plan, **want) -> None:
    for ch in plan:
        for k, v in want.items():
            assert ch[k] == v, (k, v, plan)


# ---- batch 1, fused attention + o_proj --------------------------------------------------------------------------------------

FUSED = [("d128g1", True, True), ("d128g2", True, True), ("d128g2", False, True), ("d128g4", True, True),
         ("d128g1", True, False), ("d128g2", True, False), ("d128g2", False, False), ("d128g4", True, False),
         ("d64g2", True, True), ("d64g2", False, True)]


@pytest.mark.parametrize("shape,qk,mfma", FUSED)
def test_batch1_fused_attention(shape, qk, mfma):
    """attn_oproj_mfma_kernel, attn_oproj_kernel under PGK_ATTN_MFMA=0, and head_dim 64 (always dot2): every context where
    the staging, the preload or the tile walk changes shape, up to the last fused position 383."""
    r = rig(shape, qk, env=() if mfma else (("PGK_ATTN_MFMA", "0"),))
    kernel = "attn_oproj_mfma" if (mfma and r.p.D == 128) else "attn_oproj"
    for pos in R.FUSED_CTX:
        assert_plan(r.plan([pos]), attn=kernel, form="gemv", m=1, tail="none")
        r.step([pos], what=kernel)
        assert r.eng.launches_per_step() == 4 + 2
    assert_plan(r.plan([384]), attn="attn_decode_split")        # SHORT_CTX_B1: position 384 leaves the fused kernel


@pytest.mark.parametrize("shape,qk,mfma", [f for f in FUSED if f[1]])
def test_batch1_fused_attention_keys_in_the_middle(shape, qk, mfma):
    """The top height planted once in every position group (16 rows; 32 at head_dim 64) of the contexts around the 128-row
    staging edge, the 192-row chunk / preload edge and the last fused position."""
    r = rig(shape, qk, env=() if mfma else (("PGK_ATTN_MFMA", "0"),))
    for pos in R.PLANT_CTX:
        for m in R.plant_rows_short(pos, r.p.D):
            r.step_planted(pos, m, what=("fused", pos))


# ---- batch 1 and 2, split-KV ----------------------------------------------------------------------------------------------

SPLIT = [("d128g2", True), ("d128g2", False), ("d128g1", True), ("d128g4", True), ("d64g2", True)]


@pytest.mark.parametrize("merged", [True, False])
@pytest.mark.parametrize("shape,qk", SPLIT)
def test_split_kv_one_and_two_sequences(shape, qk, merged):
    """attn_decode_kernel slices + attn_merge_oproj_kernel (bf16 W_o), and under PGK_MERGED_OPROJ=0 attn_merge_kernel + the
    o_proj GEMV, on a 4096-row cache: the first split position, SHORT_CTX, and both sides of every context tier."""
    r = rig(shape, qk, cache=R.CACHE_LONG, max_batch=2, env=() if merged else (("PGK_MERGED_OPROJ", "0"),))
    tail = "merge_oproj_bf16" if merged else "merge"
    for i, pos in enumerate(R.SPLIT_CTX):
        plan = r.plan([pos])
        assert_plan(plan, attn="attn_decode_split", form="gemv", m=1, tail=tail)
        assert plan[0]["span"] == (1024 if pos < 1024 else 2048 if pos < 2048 else 4096), plan
        r.step([pos], what=tail)
        assert r.eng.launches_per_step() == (5 if merged else 6) + 2
        other = R.SPLIT_CTX[(i + 5) % len(R.SPLIT_CTX)]
        if max(pos, other) > 512:
            assert_plan(r.plan([pos, other]), attn="attn_decode_split", form="gemv", m=2, tail=tail)
            r.step([pos, other], what=(tail, "two sequences"))


@pytest.mark.parametrize("shape,qk,merged", [("d128g2", True, True), ("d128g2", True, False), ("d64g2", True, True), ("d128g4", True, True)])
def test_split_kv_first_and_last_row_of_every_slice(shape, qk, merged):
    """The top height at the first and the last row of every split-KV slice of the step (slices are cut by absolute position
    over the step's tier): a slice that is dropped, merged with a zero weight or cut one row short loses exactly these."""
    r = rig(shape, qk, cache=R.CACHE_LONG, max_batch=2, env=() if merged else (("PGK_MERGED_OPROJ", "0"),))
    for pos in (385, 1025, 2049, 4094):
        ch = r.plan([pos])[0]
        assert ch["attn"] == "attn_decode_split" and ch["nsplit"] > 1
        for m in R.slice_edge_rows(pos, ch["span"], ch["nsplit"], r.p.D):
            r.step_planted(pos, m, what=("split", ch["nsplit"], "slices of", ch["span"]))


@pytest.mark.parametrize("shape,qk", [("d128g2", True), ("d64g2", True), ("d128g2", False)])
def test_split_kv_at_short_contexts(shape, qk):
    """PGK_FUSED_ATTN=0: the split-KV sequence at the contexts the fused and whole-context kernels normally take."""
    r = rig(shape, qk, cache=R.CACHE_LONG, max_batch=2, env=(("PGK_FUSED_ATTN", "0"),))
    for i, pos in enumerate(R.SPLIT_SHORT_CTX):
        assert_plan(r.plan([pos]), attn="attn_decode_split", tail="merge_oproj_bf16")
        r.step([pos], what="split at a short context")
        other = R.SPLIT_SHORT_CTX[(i + 4) % len(R.SPLIT_SHORT_CTX)]
        assert_plan(r.plan([pos, other]), attn="attn_decode_split", m=2)
        r.step([pos, other], what="split at short contexts, two sequences")
    for m in R.slice_edge_rows(383, r.plan([383])[0]["span"], r.plan([383])[0]["nsplit"], r.p.D):
        r.step_planted(383, m, what="split at a short context")


# ---- batches ----------------------------------------------------------------------------------------------------------------

def batch_positions(B: int, shift: int = 0) -> list[int]:
    """Every sequence its own position, straddling 191 / 192 / 193, 383 / 384 and up to 511, the last position of the short
    sequence (context 512 with the new token).  The list moves on by one for every 16 sequences: no two sequences of a batch
    of up to 64 share both tag (slot % 4) and position, so a sequence slot that is off by any stride returns another row."""
    short = R.BATCH_CTX
    assert len(short) == 16 and max(short) <= 511
    pos = [short[(b + b // 16 + shift) % 16] for b in range(B)]
    assert len({(b % R.NTAGS, q) for b, q in enumerate(pos)}) == B
    return pos


def chunk_forms(plan):
    return [(ch["form"], ch["m"]) for ch in plan]


BATCH_SHAPES = [("d128g2", True), ("d128g2", False), ("d128g4", True), ("d64g2", True)]


@pytest.mark.parametrize("shape,qk", BATCH_SHAPES)
def test_batches_whole_context_attention(shape, qk):
    """2 and 4 sequences (GEMV chunks), 3, 5 and 16 (batched MFMA), 17 and 33 (packed): whole-context attention with each
    sequence at its own context - attn_oproj_mfma_kernel<OPROJ = false> at head_dim 128 (fp32 rows for the GEMV chunks,
    bf16 rows for the MFMA o_proj), attn_decode_kernel<DIRECT> at head_dim 64."""
    r = rig(shape, qk, cache=1024, max_batch=33)
    direct = "attn_mfma_direct" if r.p.D == 128 else "attn_decode_direct"
    for B, forms in ((2, [("gemv", 2)]), (4, [("gemv", 4)]), (3, [("batched", 3)]), (5, [("batched", 5)]), (16, [("batched", 16)]),
                     (17, [("packed", 17)]), (33, [("packed", 33)])):
        for shift in (0, 5):
            pos = batch_positions(B, shift)
            plan = r.plan(pos)
            assert chunk_forms(plan) == forms, plan
            assert_plan(plan, attn=direct, nsplit=1, tail="none", out="f32" if forms[0][0] == "gemv" else "bf16")
            r.step(pos, what=(direct, B))


@pytest.mark.parametrize("shape,qk", [("d128g2", True), ("d128g4", True)])
def test_batches_on_the_dot2_whole_context_kernel_and_gemv_chunks(shape, qk):
    """PGK_ATTN_MFMA=0 + PGK_BATCHED_MFMA=0: attn_decode_kernel<DIRECT> at head_dim 128 with fp32 rows, in GEMV chunks of
    8 / 4 / 2 / 1 sequences (8, 7 = 4 + 2 + 1 and 13 = 8 + 4 + 1: the single sequence takes the fused kernel)."""
    r = rig(shape, qk, cache=1024, max_batch=16, env=(("PGK_ATTN_MFMA", "0"), ("PGK_BATCHED_MFMA", "0")))
    for B, forms in ((8, [8]), (7, [4, 2, 1]), (13, [8, 4, 1])):
        pos = batch_positions(B, 2)
        plan = r.plan(pos)
        assert [ch["m"] for ch in plan] == forms and all(ch["form"] == "gemv" for ch in plan), plan
        for ch in plan:
            assert ch["attn"] == ("attn_oproj" if ch["m"] == 1 else "attn_decode_direct") and ch["out"] == "f32", plan
        r.step(pos, what=("gemv chunks", B))


@pytest.mark.parametrize("shape,qk", [("d128g2", True), ("d64g2", True)])
def test_batches_on_the_dot2_whole_context_kernel_bf16_rows(shape, qk):
    """attn_decode_kernel<DIRECT> writing bf16 rows for the batched, tiled (PGK_PACKED_DECODE=0) and packed o_proj."""
    for env in ((("PGK_ATTN_MFMA", "0"),), (("PGK_ATTN_MFMA", "0"), ("PGK_PACKED_DECODE", "0"))):
        r = rig(shape, qk, cache=1024, max_batch=33, env=env)
        big = "tiled" if len(env) == 2 else "packed"
        for B, form in ((3, "batched"), (16, "batched"), (17, big), (33, big)):
            pos = batch_positions(B, 7)
            plan = r.plan(pos)
            assert chunk_forms(plan) == [(form, B)], plan
            assert_plan(plan, attn="attn_decode_direct", out="bf16", tail="none")
            r.step(pos, what=(form, B))


@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("shape,qk", [("d128g2", True), ("d64g2", True)])
def test_batches_with_one_long_sequence_take_the_split_sequence(shape, qk, packed):
    """One context beyond SHORT_CTX turns the whole step to split-KV slices + attn_merge_kernel, for every chunk form; the
    MFMA whole-context kernel stays asserted for the same batches just below (largest context 512)."""
    r = rig(shape, qk, cache=1024, max_batch=33, env=() if packed else (("PGK_PACKED_DECODE", "0"),))
    for B in (2, 4, 3, 8, 16, 17, 33):
        pos = batch_positions(B, 3)
        pos[B // 2] = 513 if B % 2 else 1000
        plan = r.plan(pos)
        assert_plan(plan, attn="attn_decode_split")
        assert all(ch["tail"] == ("merge_oproj_bf16" if ch["m"] <= 2 and ch["form"] == "gemv" else "merge") for ch in plan), plan
        if B > 16:
            assert plan[0]["form"] == ("packed" if packed else "tiled"), plan
        r.step(pos, what=("one long sequence", B))


# ---- GQA group 7: head-chunk launches ---------------------------------------------------------------------------------------

def test_gqa_group_of_seven_runs_three_head_chunk_launches():
    """28 / 4-style groups: launches of 4 + 2 + 1 query heads per kv head (g_off / g_total), split (one sequence: no fused
    or merged form; two sequences at long contexts) and whole-context (two sequences at short contexts)."""
    r = rig("d128g7", True, cache=R.CACHE_LONG, max_batch=2)
    for pos in (1, 16, 191, 192, 193, 383, 384, 513, 1024, 1025, 4095):
        assert_plan(r.plan([pos]), attn="attn_decode_split", heads="4+2+1", tail="merge")
        r.step([pos], what="group 7, split")
        assert r.eng.launches_per_step() == 8 + 2        # qkv, 3 attention launches, merge, o_proj, gate_up, down
    for pos in ([191, 192], [193, 16], [510, 383], [1, 511]):
        assert_plan(r.plan(pos), attn="attn_decode_direct", heads="4+2+1", tail="none", m=2)
        r.step(pos, what="group 7, whole context")
    for pos in ([513, 192], [4094, 1025]):
        assert_plan(r.plan(pos), attn="attn_decode_split", heads="4+2+1", tail="merge", m=2)
        r.step(pos, what="group 7, split, two sequences")
    ch = r.plan([1025])[0]
    for m in R.slice_edge_rows(1025, ch["span"], ch["nsplit"], 128):
        r.step_planted(1025, m, what="group 7, split")


# ---- captured steps -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,qk", [("d128g2", True), ("d64g2", False)])
def test_captured_steps_follow_the_context_tier(shape, qk):
    """capture + set_state + replay(1): the fused tier, the move to the 1024 tier at position 384, to the 2048 tier at 1024,
    to the cache-length tier at 2048 - each replay reads the winner of ITS context, and the launch count names the tier."""
    r = rig(shape, qk, cache=R.CACHE_LONG, max_batch=1)
    for pos in (100, 191, 383, 384, 385, 1023, 1024, 1025, 2047, 2048, 4095, 192, 1024):
        ch = r.plan([pos])[0]
        fused = pos + 1 <= 384
        assert ch["attn"] == (("attn_oproj_mfma" if r.p.D == 128 else "attn_oproj") if fused else "attn_decode_split")
        if not fused:
            assert ch["span"] == (1024 if pos < 1024 else 2048 if pos < 2048 else 4096)
        r.step([pos], replay=True, what=("replay", ch["attn"], ch["span"]))
        assert r.eng.launches_per_step() == (4 if fused else 5) + 2
    for pos, m in ((383, 200), (1025, 1023), (1025, 0), (2049, 2047), (2049, 1024)):
        r.step_planted(pos, m, replay=True, what="replay")


# ---- prefill --------------------------------------------------------------------------------------------------------------------

def run_prefill(r: Rig, n: int, kind: str, chunks) -> None:
    p, eng = r.p, r.eng
    toks, winner = R.prefill_prompt(n, kind)
    got, last = [], None
    for a, ln in chunks:
        buf = zeros((ln, R.VOCAB), bfloat16)
        last = eng.prefill(toks[a:a + ln], seq=0, start_pos=a, all_logits=buf)
        got.append(O.bf16_bits_to_f32(buf.to_numpy()))
    got = np.concatenate(got)
    r.check_cache_rows(0, 0, toks, ("prefill", n, kind, len(chunks), "chunks"))
    v = O.bf16_bits_to_f32(r.rows_words(0, 0, n)[1]).transpose(1, 0, 2)     # [n, Hkv, D] as written
    for i in range(n):
        want = p.logits_from_v(toks[i], v[winner[i]])
        bad = np.abs(got[i, :p.H].astype(F64) - want) > p.logit_bar(want, 1)
        if bad.any() or got[i, p.H:].any() or not np.isfinite(got[i]).all():
            raise AssertionError(f"prefill of {n} {kind} tokens in chunks {chunks}: row {i} expected row {winner[i]}; {r.explain(0, toks[i], got[i])}")
    want = p.logits_from_v(toks[n - 1], v[winner[n - 1]])
    assert (np.abs(last[:p.H].astype(F64) - want) <= p.logit_bar(want, 1)).all() and not last[p.H:].any(), ("last-row fp32 logits", n, kind)
    eng.prefill(r.fill[0][:n], seq=0, want_last_logits=False)               # the ascending fill back


@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("shape,qk", [("d128g2", True), ("d128g2", False), ("d64g2", True)])
def test_prefill_rows_return_their_own_key(shape, qk, packed):
    """One-shot prompts and the same prompts in ragged chunks (start_pos > 0), through the all_logits buffer (bf16: the
    normalised row's rounding is the only one, the identity lm_head returns bf16 values) and the fp32 last row, with and
    without the packed weight copy.  Ascending heights: row i returns row i; descending behind five ascending rows: every
    later row returns row 4 of the FIRST chunk.  The rows beyond the prompt hold higher heights (the fill): a row that sees
    past its position returns one of those."""
    r = rig(shape, qk, cache=1024, max_batch=1, env=() if packed else (("PGK_PACKED_PREFILL", "0"),))
    for n in R.PREFILL_LENS:
        for kind in ("ascending", "descending"):
            run_prefill(r, n, kind, [(0, n)])
            if n > R.PREFILL_CHUNKS[0]:
                run_prefill(r, n, kind, R.prefill_chunks(n))


# ---- fp8 weights (w8a16) ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,qk", R.FP8_PROBES)
def test_fp8_split_kv_with_the_merged_fp8_o_proj(shape, qk):
    """attn_decode_kernel slices + attn_merge_oproj_kernel<FP8> (16 codes per lane, block scale per lane), one and two
    sequences.  fp8 engines have no fused kernel, so one sequence takes this path at SHORT contexts as well."""
    r = rig(shape, qk, cache=R.CACHE_LONG, max_batch=2, fp8=True)
    for i, pos in enumerate((1, 191, 192, 193, 383, 384) + R.SPLIT_CTX):
        assert_plan(r.plan([pos]), attn="attn_decode_split", form="gemv", m=1, tail="merge_oproj_fp8")
        r.step([pos], what="merge_oproj_fp8")
        assert r.eng.launches_per_step() == 5 + 2
        other = R.SPLIT_CTX[(i + 5) % len(R.SPLIT_CTX)]
        if max(pos, other) > 512:
            assert_plan(r.plan([pos, other]), attn="attn_decode_split", form="gemv", m=2, tail="merge_oproj_fp8")
            r.step([pos, other], what=("merge_oproj_fp8", "two sequences"))
    for pos in (383, 1025, 4094):
        ch = r.plan([pos])[0]
        for m in R.slice_edge_rows(pos, ch["span"], ch["nsplit"], r.p.D):
            r.step_planted(pos, m, what=("merge_oproj_fp8", ch["nsplit"], "slices of", ch["span"]))


@pytest.mark.parametrize("shape,qk", R.FP8_PROBES)
def test_fp8_gemv_chunks(shape, qk):
    """fp8 GEMV projections around whole-context attention (chunks of 2 and 4 at short contexts), the split sequence with
    attn_merge_kernel + the fp8 o_proj GEMV (PGK_MERGED_OPROJ=0; chunks of 4 and 8 + 1 at a long context)."""
    r = rig(shape, qk, cache=1024, max_batch=33, fp8=True)
    direct = "attn_mfma_direct" if r.p.D == 128 else "attn_decode_direct"
    for B in (2, 4):
        for shift in (0, 9):
            pos = batch_positions(B, shift)
            plan = r.plan(pos)
            assert chunk_forms(plan) == [("gemv", B)], plan
            assert_plan(plan, attn=direct, out="f32", tail="none")
            r.step(pos, what=("fp8 gemv chunk", B))
    pos = batch_positions(4, 3)
    pos[1] = 1000
    assert_plan(r.plan(pos), attn="attn_decode_split", form="gemv", m=4, tail="merge")
    r.step(pos, what="fp8 gemv chunk of 4, split")
    r2 = rig(shape, qk, cache=R.CACHE_LONG, max_batch=2, env=(("PGK_MERGED_OPROJ", "0"),), fp8=True)
    for pos in (192, 385, 1024, 2049, 4095):
        assert_plan(r2.plan([pos]), attn="attn_decode_split", tail="merge")
        r2.step([pos], what="fp8 merge + o_proj GEMV")
        assert r2.eng.launches_per_step() == 6 + 2


@pytest.mark.parametrize("shape,qk", R.FP8_PROBES)
def test_fp8_batched_chunks(shape, qk):
    """3, 5, 16 sequences on the batched fp8 MFMA projections, 17 and 33 in one chunk, whole-context attention with bf16 rows;
    the same batches with one long sequence (split-KV + attn_merge_kernel)."""
    r = rig(shape, qk, cache=1024, max_batch=33, fp8=True)
    direct = "attn_mfma_direct" if r.p.D == 128 else "attn_decode_direct"
    for B in (3, 5, 16, 17, 33):
        pos = batch_positions(B, 4)
        plan = r.plan(pos)
        assert [ch["m"] for ch in plan] == [B] and plan[0]["form"] == ("batched" if B <= 16 else "packed"), plan
        assert_plan(plan, attn=direct, out="bf16", tail="none")
        r.step(pos, what=("fp8", plan[0]["form"], B))
        pos[B // 2] = 513
        assert_plan(r.plan(pos), attn="attn_decode_split", tail="merge")
        r.step(pos, what=("fp8, one long sequence", B))


def test_fp8_prefill_rows_return_their_own_key():
    """The prompts of test_prefill_rows_return_their_own_key on a w8a16 engine (the dequantised packed copy)."""
    r = rig("d128g2", True, cache=1024, max_batch=1, fp8=True)
    for n in R.PREFILL_LENS:
        for kind in ("ascending", "descending"):
            run_prefill(r, n, kind, [(0, n)])
            if n > R.PREFILL_CHUNKS[0]:
                run_prefill(r, n, kind, R.prefill_chunks(n))
