"""CPU side of the engine's exact visible-key checks (tests/engine_stair_ref.py; GPU side: tests/test_engine_stair_gpu.py).

1. Precondition: on every probe model the GPU tests use, at every context they use, the fp64 oracle
   (oracle.cpu_ref.build_qwen3_ref with the explicit lm_head) returns the expected V row within 2**-20 in every element -
   decode steps over the ascending fill, decode steps with the top height planted in the middle, and the ascending /
   descending prompts of the prefill tests.
2. Contrast: a mask one key short, one (stale) key long, and without a whole 64-row slice - on a random-weight model the
   whole-vector bar of tests/test_gpu_model.py (rel_err < 1e-2) passes a single key, and a slice with small weights at long
   context; on the probe model each returns another V row.  The figures are printed (pytest -s) and recorded in DESIGN.md 4.1.
3. The derived bar: an fp32 emulation of the readout in two summation orders stays inside logit_bar.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest

from oracle import cpu_ref as O
from tests import engine_stair_ref as R
from tests.conftest import rel_err

F32, F64 = np.float32, np.float64
N = R.CACHE_LONG


@functools.lru_cache(maxsize=None)
def oracle_of(shape: str, qk: bool, tag: int = 0, fp8: bool = False):
    """(probe, oracle model, cache of the ascending fill, cache of the top token at every row): built once, read-only.
    fp8: the oracle runs on the DEQUANTISED weights of the hand-encoded w8a16 probe."""
    p = R.probe(shape, qk, fp8)
    ref = R.oracle_model(p.cfg, p.weights, N)
    fill = R.oracle_cache(ref, R.fill_tokens(N, tag))
    top = R.oracle_cache(ref, [int(R.token(R.TOP, tag))] * N)      # the top token's K / V row at every position
    for k, v in fill + top:
        k.setflags(write=False)
        v.setflags(write=False)
    return p, ref, fill, top


ALL_PROBES = [(s, q, False) for s, q in R.PROBES] + [(s, q, True) for s, q in R.FP8_PROBES]


@pytest.mark.parametrize("shape,qk,fp8", ALL_PROBES)
def test_probe_construction(shape, qk, fp8):
    """RoPE leaves the stair columns alone at every position of the longest cache, kappa's bf16 word does not depend on
    the order of fp32 arithmetic, and the oracle's cache rows are the closed forms the GPU tests compare with."""
    p, ref, fill, _ = oracle_of(shape, qk, 0, fp8)
    p.check_rope(N)
    p.check_k_word()
    toks = R.fill_tokens(N)
    k, v = fill[0]
    assert np.abs(v - p.v_rows(toks)).max() < R.PRECONDITION
    bits = p.k_expected_bits(toks)
    for kvh in range(p.Hkv):
        got = k[:, kvh][:, np.concatenate([p.bit_cols, p.cmp_cols])]
        assert np.abs(got[bits == 1] - p.kappa).max() < R.PRECONDITION
        assert np.abs(got[bits == 0]).max() <= p.k_zero_bound(N)
    # every K row has one norm in front of QK-norm: 12 set bits or complements + D - 24 noise entries, all of magnitude 1
    sq = ((p.x(toks) @ p.weights["layers"][0]["k"].astype(F64).T) ** 2).reshape(N, p.Hkv, p.D).sum(-1)
    assert np.all(sq == p.D - R.NBITS)


@pytest.mark.parametrize("shape,qk,fp8", ALL_PROBES)
def test_precondition_decode_contexts(shape, qk, fp8):
    """Decode of a height-0 token at every context the GPU tests use: the oracle returns cache row p - 1 (p = 0: the
    token's own row), for two slots."""
    worst = 0.0
    for tag in (0, 3):
        p, ref, fill, _ = oracle_of(shape, qk, tag, fp8)
        v = fill[0][1]
        tok = int(R.token(0, tag))
        for pos in R.ALL_CTX:
            got = R.oracle_step(ref, fill, tok, pos)
            want = p.logits_from_v(tok, v[pos - 1] if pos else p.v_rows([tok])[0])
            worst = max(worst, float(np.abs(got[:p.H] - want).max()))
            assert np.abs(got[p.H:]).max() == 0.0
    print(shape, qk, "decode precondition, worst element", worst)
    assert worst < R.PRECONDITION


@pytest.mark.parametrize("shape,qk,fp8", ALL_PROBES)
def test_precondition_planted_rows(shape, qk, fp8):
    """The top height planted at row m wins at every later context: every plant the GPU tests make at a short context and
    a sample of the long ones."""
    p, ref, fill, top = oracle_of(shape, qk, 0, fp8)
    tok = int(R.token(0, 0))
    worst = 0.0
    cases = [(pos, m) for pos in R.PLANT_CTX for m in R.plant_rows_short(pos, p.D)]
    cases += [(pos, m) for pos in (1025, 4094) for m in (0, 63, 64, pos // 2, pos - 2)]
    for pos, m in cases:
        past = [(k.copy(), v.copy()) for k, v in fill]
        past[0][0][m], past[0][1][m] = top[0][0][m], top[0][1][m]
        got = R.oracle_step(ref, past, tok, pos)
        want = p.logits_from_v(tok, top[0][1][m])
        worst = max(worst, float(np.abs(got[:p.H] - want).max()))
    print(shape, qk, len(cases), "plants, worst element", worst)
    assert worst < R.PRECONDITION


@pytest.mark.parametrize("shape,qk,fp8", [("d128g2", True, False), ("d128g2", False, False), ("d64g2", True, False), ("d128g2", True, True)])
def test_precondition_prefill_prompts(shape, qk, fp8):
    """Ascending prompts: row i returns its own V row.  Descending rows behind an ascending first chunk: the first chunk's
    top row."""
    p = R.probe(shape, qk, fp8)
    ref = R.oracle_model(p.cfg, p.weights, 1024)
    for n in R.PREFILL_LENS:
        for kind in ("ascending", "descending"):
            toks, winner = R.prefill_prompt(n, kind)
            hidden, _ = ref(toks)
            got = np.asarray(ref.get_logits(hidden))
            v = p.v_rows(toks)
            want = np.stack([p.logits_from_v(toks[i], v[winner[i]]) for i in range(n)])
            assert np.abs(got[:, :p.H] - want).max() < R.PRECONDITION, (n, kind)
            assert np.abs(got[:, p.H:]).max() == 0.0


@pytest.mark.parametrize("shape,qk", R.FP8_PROBES)
def test_fp8_probe_weights_are_exact_under_power_of_two_block_scales(shape, qk):
    """The w8a16 probe: every block scale is a power of two, decoding the codes the engine gets (the oracle's e4m3 table times
    the scale) gives the model's weights bit for bit, these are bf16 values (so the kernels that round the dequantised weight
    to bf16 and those that multiply lut * scale in fp32 see one matrix), and the stair, the copying W_k and the identity W_o
    are those of the bf16 probe."""
    p, b = R.probe(shape, qk, True), R.probe(shape, qk, False)
    lw, bw = p.weights["layers"][0], b.weights["layers"][0]
    fused = {"w_qkv": np.concatenate([lw["q"], lw["k"], lw["v"]]), "w_o": lw["o"], "w_gate_up": np.concatenate([lw["gate"], lw["up"]]), "w_down": lw["down"]}
    for name, (codes, sbits) in p.fp8.items():
        scale = O.bf16_bits_to_f32(sbits)
        m, e = np.frexp(scale)
        assert np.all(m == 0.5), name
        deq = O.dequantize_fp8_e4m3_block(codes, sbits)
        assert np.array_equal(deq, fused[name]) and np.array_equal(O.bf16_round(deq), deq), name
        assert np.array_equal(O.dequantize_fp8_e4m3_block_w8a16_gemm(codes, sbits), deq), name
    assert np.array_equal(lw["k"], bw["k"]) and np.array_equal(lw["o"], bw["o"]) and not lw["down"].any()
    for h in range(p.Hq):
        assert np.array_equal(lw["q"][h * p.D + p.bit_cols], bw["q"][h * p.D + p.bit_cols])
    assert p.kappa == b.kappa and p.step_lo == b.step_lo


# ---- contrast ---------------------------------------------------------------------------------------------------------

CONTRAST_CTX = 4000
MUTATIONS = {"one key short": lambda pos: np.arange(pos - 1), "one stale key long": lambda pos: np.arange(pos + 1),
             "64-row slice removed": lambda pos: np.r_[0:128, 192:pos]}


@functools.lru_cache(maxsize=None)
def random_model(std: float):
    cfg = dict(vocab_size=2048, hidden_size=256, num_layers=2, num_heads=2, num_kv_heads=1, head_dim=128, intermediate_size=256,
               rope_theta=1e6, norm_eps=1e-6)
    w = O.make_qwen3_weights(cfg, seed=61, std=std)
    ref = R.oracle_model(cfg, w, N)
    toks = [int(t) for t in np.random.default_rng(62).integers(0, cfg["vocab_size"], N)]
    return ref, toks, R.oracle_cache(ref, toks)


# (weight scale, context) -> does the whole-vector bar see a lost 64-row slice there?  A single key it never sees.
SLICE_SEEN = {(0.005, 4000): False, (0.005, 1024): True, (0.005, 320): True, (0.02, 4000): True, (0.02, 1024): True, (0.02, 320): True}
ONE_KEY_SEEN = {(0.02, 320): True}          # everywhere else a single key stays under the bar


def test_contrast_whole_vector_bar_on_random_weights():
    """The three mask mutations on random-weight models (2 layers, Qwen3 wiring; N(0, 0.02**2), the weights of
    tests/test_gpu_model.py and tests/test_gpu_attn_fused_trim.py, and N(0, 0.005**2)) at contexts 320, 1024 and 4000,
    against the rel_err < 1e-2 bar those suites assert.  Every figure is asserted on the side it falls, so none can drift:

      * one key short / one stale key long stay UNDER the bar at context 1024 and 4000 for both weight scales
        (2e-4 .. 6e-3) and at context 320 for the small weights: the old bar is blind to a single key;
      * at context 320 with the suites' weights a single key moves the logits by 2e-2 .. 3e-2: there the old bar sees it;
      * a lost 64-row slice stays under the bar only with small weights at long context (5e-3 at std 0.005, context 4000);
        at std 0.005 / context 1024 (1.9e-2) and with the suites' weights (2e-2 at 4000, 9e-2 at 1024) the bar DOES see it.

    The probe model (next test) sees every one of them at any context."""
    for std in (0.005, 0.02):
        ref, toks, past = random_model(std)
        for pos in (CONTRAST_CTX, 1024, 320):
            base = R.oracle_step(ref, past, toks[pos], pos)
            for name, rows in MUTATIONS.items():
                err = rel_err(R.oracle_step(ref, past, toks[pos], pos, rows(pos)), base)
                seen = SLICE_SEEN[(std, pos)] if "slice" in name else ONE_KEY_SEEN.get((std, pos), False)
                print(f"random weights std {std} context {pos}: {name}: rel_err {err:.2e} ({'seen' if seen else 'unseen'} by the 1e-2 bar)")
                assert (err > 1e-2) if seen else (err < 1e-2), (std, pos, name, err)


@pytest.mark.parametrize("shape,qk", [("d128g2", True), ("d64g2", False)])
def test_contrast_probe_model_returns_another_row(shape, qk):
    """The same mutations on the probe model: each returns a different V row, far outside the derived bar, and
    nearest_row names the row.  The slice case plants the top height inside the slice that is then removed."""
    p, ref, fill, top = oracle_of(shape, qk)
    tok = int(R.token(0, 0))
    for pos in (300, CONTRAST_CTX):
        v = fill[0][1]
        want = p.logits_from_v(tok, v[pos - 1])
        cache = v.transpose(1, 0, 2)[None]
        for name, rows, row_seen in (("one key short", np.arange(pos - 1), pos - 2), ("one stale key long", np.arange(pos + 1), pos)):
            got = R.oracle_step(ref, fill, tok, pos, rows)[:p.H]
            excess = float((np.abs(got - want) / p.logit_bar(want, 1)).max())
            who = R.nearest_row(p, tok, got, cache)
            print(f"probe {shape} qk_norm={qk} context {pos}: {name}: worst element {excess:.1e} x the bar, nearest row {who[:3]}")
            assert excess > 100 and who[:3] == (0, 0, row_seen)
        m = 150
        past = [(k.copy(), v2.copy()) for k, v2 in fill]
        past[0][0][m], past[0][1][m] = top[0][0][m], top[0][1][m]
        want = p.logits_from_v(tok, top[0][1][m])
        assert np.abs(R.oracle_step(ref, past, tok, pos)[:p.H] - want).max() < R.PRECONDITION
        got = R.oracle_step(ref, past, tok, pos, np.r_[0:128, 192:pos])[:p.H]
        excess = float((np.abs(got - want) / p.logit_bar(want, 1)).max())
        who = R.nearest_row(p, tok, got, past[0][1].transpose(1, 0, 2)[None])
        print(f"probe {shape} qk_norm={qk} context {pos}: 64-row slice removed: worst element {excess:.1e} x the bar, nearest row {who[:3]}")
        assert excess > 100 and who[:3] == (0, 0, pos - 1)


# ---- the derived bar ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["d128g1", "d128g4", "d128g7"])
def test_derived_bar_holds_in_fp32_in_two_summation_orders(shape):
    """The readout in fp32, with the sum of squares taken sequentially and in 64 interleaved lanes + a tree (the two
    extremes of what a kernel does), with and without the bf16 rounding of the normalised row, against float64."""
    p = R.probe(shape, True)
    rng = np.random.default_rng(3)
    worst = 0.0
    for tok in rng.integers(0, R.VOCAB, 64):
        v16 = O.bf16_round(p.v_rows([int(rng.integers(0, R.VOCAB))])[0].astype(F32))
        want = p.logits_from_v(int(tok), v16)
        h = (p.weights["embed"][tok] + np.repeat(v16, p.G, axis=0).reshape(p.H)).astype(F32)
        sq = h * h
        seq = F32(0)
        for t in sq:
            seq = F32(seq + t)
        lanes = sq.reshape(-1, 64).sum(axis=0, dtype=F32)
        while lanes.size > 1:
            lanes = (lanes[0::2] + lanes[1::2]).astype(F32)
        for ss in (seq, lanes[0]):
            inv = F32(1.0) / np.sqrt(F32(ss / F32(p.H)) + F32(R.EPS), dtype=F32)
            y = (h * inv).astype(F32)
            for n_bf16, got in ((0, y), (1, O.bf16_round(y))):
                ratio = float((np.abs(got.astype(F64) - want) / p.logit_bar(want, n_bf16)).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, (shape, int(tok), n_bf16, ratio)
    print(shape, "fp32 emulation: worst element", worst, "of the bar")
