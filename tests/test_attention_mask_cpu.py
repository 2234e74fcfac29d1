"""CPU side of the exact causal-mask tests (tests/attn_stair_ref.py has the construction).

  * precondition: for every case the GPU file runs, the op's own fp64 oracle on the rounded staircase inputs returns the
    expected V rows within 2**-20 in every element;
  * sensitivity: the same reference with its mask shifted by +1 / -1, on all rows and on tile-edge rows only, returns rows
    that the exact comparison rejects - the neighbouring V rows - and moves the suite's whole-tensor rel_err by order 1;
  * contrast: on random data the tile-edge leak stays under the suite's 1e-2 bar, which is why the exact tests exist.
"""

from __future__ import annotations

import math

import numpy as np
import pytest

from oracle import cpu_ref as O
from tests import attn_stair_ref as S
from tests import fp8_attn_ref as F8
from tests import llama4_ref as R
from tests import posenc_ref as P
from tests.conftest import rel_err

IROPE_ATTN_SCALE, IROPE_FLOOR_SCALE, IROPE_START = 0.1, 16.0, 100      # as the GPU file: positions start above floor_scale


def _dense_oracle(c: S.Stair) -> np.ndarray:
    q, k, v = c.f64()
    return O.sdpa_causal(q, np.repeat(k, c.rep, axis=0), np.repeat(v, c.rep, axis=0), 1.0)


DENSE = ([t + (dt,) for t in S.FLASH2 for dt in ("bf16", "f16")] + [t + ("bf16",) for t in S.ONE_TILE] + S.GEN1 + S.NAIVE
         + [S.NAIVE_ENV])


def test_no_case_exceeds_the_length_limit():
    dense = DENSE + [t + ("bf16",) for t in S.FP8] + [t[:6] for t in S.IROPE] + S.ALIBI
    assert max(t[3] for t in dense) <= S.MAX_KV
    assert max(m for m, _ in S.DECODE_CTX) <= S.MAX_KV and S.DECODE_G5[2] <= S.MAX_KV
    assert max(max(t[5]) for t in S.PAGED) <= S.MAX_KV


# ---- precondition ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", DENSE, ids=str)
def test_precondition_sdpa_causal(case):
    hq, hkv, q_len, kv_len, d, dtype = case
    c = S.make_stair(*case)
    S.check_precondition(_dense_oracle(c), c.expected(kv_len - q_len), f"sdpa_causal {case}")


@pytest.mark.parametrize("case", S.FP8, ids=str)
def test_precondition_sdpa_causal_fp8(case):
    hq, hkv, q_len, kv_len, d = case
    c = S.make_stair(*case, "bf16")
    # the quantiser keeps the staircase exactly: Q weights and K digits are powers of two / 3-bit integers times the head scale
    qd = F8.dequantize_per_head(*F8.quantize_per_head(c.q))
    kd = F8.dequantize_per_head(*F8.quantize_per_head(c.k))
    np.testing.assert_array_equal(qd[:, :, :c.nd], c.q[:, :, :c.nd])
    np.testing.assert_array_equal(kd[:, :, :c.nd], c.k[:, :, :c.nd])
    S.check_precondition(F8.sdpa_causal_fp8(c.q, c.k, c.v, 1.0), c.expected(kv_len - q_len), f"sdpa_causal_fp8 {case}")


def _irope_positions(q_len):
    return IROPE_START + np.arange(q_len, dtype=np.int64)


@pytest.mark.parametrize("case", S.IROPE, ids=str)
def test_precondition_sdpa_irope(case):
    hq, hkv, q_len, kv_len, d, dtype, small = case
    c = S.make_stair(hq, hkv, q_len, kv_len, d, dtype, S.irope_scale(d))
    pos = _irope_positions(q_len)
    assert (R.irope_temperature(pos, IROPE_ATTN_SCALE, IROPE_FLOOR_SCALE) > 1.0).all()
    offsets = [kv_len - q_len] + ([small, small + 1] if small is not None else [])
    for off in offsets:                       # small + 1: what the device sensitivity test expects (the next V rows)
        assert off + q_len <= kv_len
        got = R.sdpa_irope(c.q, c.k, c.v, pos, IROPE_ATTN_SCALE, IROPE_FLOOR_SCALE, off)
        S.check_precondition(got, c.expected(off), f"sdpa_irope {case} offset {off}")
    if small is not None:
        assert small + q_len < kv_len         # kv_seen < kv_len


@pytest.mark.parametrize("case", S.ALIBI, ids=str)
def test_precondition_sdpa_alibi(case):
    hq, hkv, q_len, kv_len, d, dtype = case
    c = S.make_stair(*case)
    S.check_precondition(P.sdpa_alibi(c.q, c.k, c.v, S.alibi_slopes(hq), 1.0), c.expected(kv_len - q_len), f"sdpa_alibi {case}")


def _decode_oracles(c: S.Stair, ctx: int, q_len: int):
    """(op name, oracle output) of the fixed-cache ops that take `scale`, over the first ctx rows of a cache that is filled
    along its whole length (sdpa_irope_fixed_cache needs inputs of its own: a larger s)."""
    hq = c.shape[0]
    q, k, v = c.f64()
    yield "sdpa_causal_fixed_cache", O.sdpa_causal_fixed_cache(q, k, v, ctx, 1.0)
    if c.dtype != "f32":
        yield "sdpa_alibi_fixed_cache", P.sdpa_alibi(q, k[:, :ctx], v[:, :ctx], S.alibi_slopes(hq), 1.0)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("hq,hc", S.DECODE_HEADS)
def test_precondition_fixed_cache(hq, hc, d, dtype):
    for max_seq, ctx in S.DECODE_CTX:
        c = S.make_stair(hq, hc, 1, max_seq, d, dtype)
        for name, got in _decode_oracles(c, ctx, 1):
            S.check_precondition(got, c.expected(ctx - 1), f"{name} ({hq},{hc}) d {d} {dtype} cache {max_seq} ctx {ctx}")
        if dtype == "bf16":
            ci = S.make_stair(hq, hc, 1, max_seq, d, dtype, S.irope_scale(d))
            got = R.sdpa_irope(ci.q, ci.k[:, :ctx], ci.v[:, :ctx], [ctx - 1], IROPE_ATTN_SCALE, IROPE_FLOOR_SCALE, ctx - 1)
            S.check_precondition(got, ci.expected(ctx - 1), f"sdpa_irope_fixed_cache ({hq},{hc}) d {d} cache {max_seq} ctx {ctx}")


def test_precondition_fixed_cache_general_path_and_five_head_groups():
    c = S.make_stair(4, 2, 5, 1024, 128, "bf16")                 # q_len 5 at ctx 75
    for name, got in _decode_oracles(c, 75, 5):
        S.check_precondition(got, c.expected(70), name + " q_len 5")
    hq, hkv, max_seq, d = S.DECODE_G5
    ctx = 1500
    c = S.make_stair(hq, hkv, 1, max_seq, d, "bf16")
    S.check_precondition(P.sdpa_alibi(c.q, c.k[:, :ctx], c.v[:, :ctx], S.alibi_slopes(hq), 1.0), c.expected(ctx - 1), "alibi G5")
    ci = S.make_stair(hq, hkv, 1, max_seq, d, "bf16", S.irope_scale(d))
    got = R.sdpa_irope(ci.q, ci.k[:, :ctx], ci.v[:, :ctx], [ctx - 1], IROPE_ATTN_SCALE, IROPE_FLOOR_SCALE, ctx - 1)
    S.check_precondition(got, ci.expected(ctx - 1), "irope G5")


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("cfg", S.PAGED, ids=str)
def test_precondition_paged_attention(cfg, dtype):
    p = S.make_paged(*cfg, dtype)
    assert (p.tables[:, -1] == 0).all() and not (p.tables[p.tables != 0] == 0).any()
    for i, ctx in enumerate(p.ctxs):                   # every page a sequence uses is its own; the rest of its row is page 0
        n = (ctx + cfg[4] - 1) // cfg[4]
        assert (p.tables[i, :n] > 0).all() and (p.tables[i, n:] == 0).all()
    used = p.tables[p.tables > 0]
    assert len(set(used.tolist())) == used.size
    got = O.paged_attention_v1(p.q.astype(np.float64), p.k, p.v, p.tables, p.ctxs, 1.0)
    S.check_precondition(got, p.expected, f"paged_attention_v1 {cfg} {dtype}")


# ---- sensitivity -------------------------------------------------------------------------------------------------------

def _edge_rows(q_len):
    return np.arange(q_len) % 64 == 63


def _check_mutations(c: S.Stair, mask_off: int, run, what: str):
    """run(last) -> fp64 attention whose row i sees keys <= last[i].  Unshifted it returns the expected rows; shifted by one
    it returns the NEIGHBOURING V rows (on every shifted row that has a neighbour), which the exact comparison rejects."""
    hq, _, q_len, kv_len, _ = c.shape
    base = mask_off + np.arange(q_len)
    want = S.to_words(c.expected(mask_off), c.dtype)
    np.testing.assert_array_equal(S.to_words(S.round_to(run(base), c.dtype), c.dtype), want)
    vexp = c.v[np.arange(hq) // c.rep]
    for shift in (+1, -1):
        for rows, floor in ((np.ones(q_len, bool), 1.0), (_edge_rows(q_len), 0.1)):
            if not rows.any():
                continue
            got = run(base + shift * rows)
            moved = rows & (base + shift >= 0) & (base + shift < kv_len)
            assert moved.any(), what
            got_w = S.to_words(S.round_to(got, c.dtype), c.dtype)
            # exactly the neighbouring V rows on the shifted rows, the expected ones elsewhere
            np.testing.assert_array_equal(got_w[:, moved], S.to_words(vexp[:, base[moved] + shift], c.dtype))
            np.testing.assert_array_equal(got_w[:, ~rows], want[:, ~rows])
            differs = (got_w != want).any(axis=2)
            assert differs[:, moved].all(), f"{what}: a row with its mask shifted by {shift} still equals the expected row"
            # replaced by independent N(0,1) rows: rel_err = sqrt(2 * fraction of rows replaced), sqrt(2) on all rows and
            # sqrt(2 / 64) = 0.18 on the tile-edge rows; the floors are well under those and 10x .. 100x the suite's 1e-2 bar
            err = rel_err(got, c.expected(mask_off))
            print(f"{what}: mask {shift:+d} on {int(rows.sum())} of {q_len} rows: rel_err {err:.3f}")
            if moved.sum() * 64 >= q_len:
                assert err >= floor, (what, shift, err)


@pytest.mark.parametrize("case", [(2, 1, 257, 400, 128, "bf16"), (4, 4, 513, 513, 64, "f16"), (8, 2, 70, 100, 128, "bf16")], ids=str)
def test_sensitivity_sdpa_causal(case):
    c = S.make_stair(*case)
    q, k, v = c.f64()
    off = case[3] - case[2]
    plain = S.attention_last(q, k, v, off + np.arange(case[2]), 1.0)
    assert np.abs(plain - _dense_oracle(c)).max() < 1e-12         # the free-mask reference IS the oracle when unshifted
    _check_mutations(c, off, lambda last: S.attention_last(q, k, v, last, 1.0), f"sdpa_causal {case}")


def test_sensitivity_sdpa_causal_fp8():
    case = (4, 2, 129, 400, 128)
    c = S.make_stair(*case, "bf16")
    qd = F8.dequantize_per_head(*F8.quantize_per_head(c.q))
    kd = F8.dequantize_per_head(*F8.quantize_per_head(c.k))
    off = case[3] - case[2]
    plain = S.attention_last(qd, kd, c.v, off + np.arange(case[2]), 1.0)
    assert np.abs(plain - F8.sdpa_causal_fp8(c.q, c.k, c.v, 1.0)).max() < 1e-12
    _check_mutations(c, off, lambda last: S.attention_last(qd, kd, c.v, last, 1.0), f"sdpa_causal_fp8 {case}")


def test_sensitivity_sdpa_irope():
    hq, hkv, q_len, kv_len, d, dtype, small = S.IROPE[1]
    c = S.make_stair(hq, hkv, q_len, kv_len, d, dtype, S.irope_scale(d))
    pos = _irope_positions(q_len)
    t = R.irope_temperature(pos, IROPE_ATTN_SCALE, IROPE_FLOOR_SCALE).astype(np.float64)
    run = lambda last: S.attention_last(c.q, c.k, c.v, last, 1.0 / math.sqrt(d), row_scale=t)      # noqa: E731
    assert np.abs(run(small + np.arange(q_len)) - R.sdpa_irope(c.q, c.k, c.v, pos, IROPE_ATTN_SCALE, IROPE_FLOOR_SCALE, small)).max() < 1e-12
    _check_mutations(c, small, run, f"sdpa_irope {S.IROPE[1]}")
    # the oracle's own offset argument, shifted
    want = S.to_words(c.expected(small), dtype)
    for shift in (+1, -1):
        got = S.to_words(S.round_to(R.sdpa_irope(c.q, c.k, c.v, pos, IROPE_ATTN_SCALE, IROPE_FLOOR_SCALE, small + shift), dtype), dtype)
        assert (got != want).any(axis=2).all()
        np.testing.assert_array_equal(got, S.to_words(c.expected(small + shift), dtype))


def test_sensitivity_sdpa_alibi():
    case = S.ALIBI[0]
    hq, hkv, q_len, kv_len, d, dtype = case
    c = S.make_stair(*case)
    sl, off = S.alibi_slopes(hq), kv_len - q_len
    run = lambda last: S.attention_last(c.q, c.k, c.v, last, 1.0, slopes=sl, origin=off)      # noqa: E731
    assert np.abs(run(off + np.arange(q_len)) - P.sdpa_alibi(c.q, c.k, c.v, sl, 1.0)).max() < 1e-12
    _check_mutations(c, off, run, f"sdpa_alibi {case}")


@pytest.mark.parametrize("ctx", [256, 257, 1023])
def test_sensitivity_fixed_cache_and_paged_context_length(ctx):
    """The oracle with context_len +-1 returns the neighbouring cache row: a kernel that reads one row past context_len, or
    stops one short, fails the exact comparison; on this data the same slip moves rel_err by order 1."""
    c = S.make_stair(4, 2, 1, 1024, 128, "bf16")
    q, k, v = c.f64()
    want = S.to_words(c.expected(ctx - 1), "bf16")
    for shift in (+1, -1):
        got = O.sdpa_causal_fixed_cache(q, k, v, ctx + shift, 1.0)
        got_w = S.to_words(S.round_to(got, "bf16"), "bf16")
        np.testing.assert_array_equal(got_w, S.to_words(c.expected(ctx - 1 + shift), "bf16"))
        assert (got_w != want).any(axis=2).all()
        assert rel_err(got, c.expected(ctx - 1)) >= 1.0


def test_sensitivity_paged_context_length_and_unused_pages():
    cfg = S.PAGED[0]
    p = S.make_paged(*cfg, "bf16")
    want = S.to_words(p.expected, "bf16")
    q = p.q.astype(np.float64)
    for shift in (+1, -1):
        ctxs = np.maximum(p.ctxs + shift, 1)
        got = O.paged_attention_v1(q, p.k, p.v, p.tables, ctxs, 1.0)
        differs = (S.to_words(S.round_to(got, "bf16"), "bf16") != want).any(axis=2)
        assert differs[ctxs != p.ctxs].all()
        assert rel_err(got, p.expected) >= 0.5          # ctx 1 cannot shrink: two of three sequences move at -1
    # a read of an unused table entry (page 0) wins the softmax: page 0 holds stairs above every valid key
    tables = p.tables.copy()
    bs = cfg[4]
    ctxs = p.ctxs.copy()
    ctxs[1] = bs + 1                                    # sequence 1 (ctx 1) now walks into its second table entry: page 0
    got = O.paged_attention_v1(q, p.k, p.v, tables, ctxs, 1.0)
    assert (S.to_words(S.round_to(got, "bf16"), "bf16")[1] != want[1]).any(axis=1).all()


# ---- contrast ----------------------------------------------------------------------------------------------------------

def test_contrast_random_data_hides_a_tile_edge_leak():
    """bf16 N(0,1) data, head_dim 128, q_len = kv_len = 300: every query row = 63 (mod 64) sees one future key - `<=` written
    for `<` in one tile's mask.  The whole-tensor measure of the rest of the suite passes it: rel_err <= 1e-2 (the max abs difference is printed)."""
    rng = np.random.default_rng(63)
    hq, q_len, kv_len, d = 4, 300, 300, 128
    q, k, v = (S.round_to(rng.standard_normal((hq, n, d)), "bf16") for n in (q_len, kv_len, kv_len))
    scale = 1.0 / math.sqrt(d)
    base = np.arange(q_len)
    good = S.attention_last(q, k, v, base, scale)
    assert np.abs(good - O.sdpa_causal(q.astype(np.float64), k.astype(np.float64), v.astype(np.float64))).max() < 1e-12
    leaky = S.attention_last(q, k, v, base + _edge_rows(q_len), scale)
    err, worst = rel_err(leaky, good), float(np.abs(leaky - good).max())
    print(f"tile-edge leak on random data: rel_err {err:.2e}, max abs {worst:.3f}")
    assert 0.0 < err <= 1e-2
