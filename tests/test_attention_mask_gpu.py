"""Exact causal-mask checks of every attention kernel on the staircase inputs of tests/attn_stair_ref.py.

Each output row must BE the V row of its last visible key: out[h, i] == V[h // rep, mask_off + i], compared on the raw
16-bit words (fp32: rtol 1e-6).  One more visible key returns the next V row, a lost key / tile / split the previous one,
a zero or a NaN, a wrong head / page / cache row some other row - on every row of every call, so one call per shape covers
every tile, wave and split edge in it.  There is no whole-tensor bar in this file; tests/test_attention_mask_cpu.py checks
on the CPU that each op's fp64 oracle returns these rows and that a mask shifted by one key does not.

Why the kernels return V unchanged: the weight of every other key is below 2**-80, 1 + 2**-80 == 1 in the kernels' fp32
sums, exp(0) == 1 exactly, the probability 1.0 is exact in bf16 / f16, and v + 2**-80 v' rounds to v in the fp32
accumulators.  The second-generation flash kernel rounds Q * scale * log2(e) (* temperature) to 16 bits first; the weights
s * 8**c share one significand, so that rounding scales the whole staircase by one factor and keeps its order.
"""

from __future__ import annotations

import numpy as np
import pytest

from tests import attn_stair_ref as S

pytestmark = pytest.mark.gpu

NAN_WORD = {"bf16": 0x7FC0, "f16": 0x7E00}
IROPE_ATTN_SCALE, IROPE_FLOOR_SCALE, IROPE_START = 0.1, 16.0, 100      # positions start above floor_scale: temperature > 1


# ---- host <-> device ---------------------------------------------------------------------------------------------------

def _dev(x, dtype):
    """float32 values of `dtype` -> device array of that dtype."""
    from pygpukit_amd.core import from_numpy

    w = S.to_words(x, dtype)
    return from_numpy(np.ascontiguousarray(w.view(np.float16) if dtype == "f16" else w))


def _raw(a):
    from pygpukit_amd.core import from_numpy

    return from_numpy(np.ascontiguousarray(a))


def _host(a, dtype) -> np.ndarray:
    """device array -> uint16 words (bf16 / f16) or float32 values."""
    h = a.to_numpy()
    return h if dtype == "f32" or h.dtype == np.uint16 else h.view(np.uint16)


def _nan_out(shape, dtype):
    """NaN everywhere: every element must be written."""
    from pygpukit_amd.core import from_numpy

    if dtype == "f32":
        return from_numpy(np.full(shape, np.nan, np.float32))
    w = np.full(shape, NAN_WORD[dtype], np.uint16)
    return from_numpy(w.view(np.float16) if dtype == "f16" else w)


def _explain(got, want, v_rows, dtype) -> str:
    """Which rows differ and which V row came back: names the key that was added or lost."""
    got2, want2 = got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1])
    bad = np.flatnonzero((got2 != want2).any(axis=1))
    lines = [f"{bad.size} of {got2.shape[0]} rows differ"]
    for r in bad[:12]:
        idx = np.unravel_index(r, got.shape[:-1])
        vr = v_rows(idx)
        hit = np.flatnonzero((vr == got2[r]).all(axis=1))
        exp = np.flatnonzero((vr == want2[r]).all(axis=1))
        back = f"V row {hit.tolist()}" if hit.size else f"no V row (first values {S.from_words(got2[r][:4], dtype)})"
        lines.append(f"  index {tuple(int(x) for x in idx)}: expected V row {exp.tolist()}, got {back}")
    return "\n".join(lines)


def _assert_rows(out, expected, dtype, v_rows):
    """out (device) equals the expected V rows: exactly on the 16-bit words, rtol 1e-6 in fp32."""
    got = _host(out, dtype)
    if dtype == "f32":
        np.testing.assert_allclose(got, expected, rtol=1e-6, atol=0.0)
        return got
    want = S.to_words(expected, dtype)
    np.testing.assert_array_equal(got, want, err_msg="" if np.array_equal(got, want) else _explain(got, want, v_rows, dtype))
    return got


def _dense_v_rows(c: S.Stair):
    vw = S.to_words(c.v, c.dtype)
    return lambda idx: vw[idx[0] // c.rep]


# ---- sdpa_causal -------------------------------------------------------------------------------------------------------

def _run_causal(case, strided=False):
    from pygpukit_amd.ops.nn.attention import sdpa_causal, sdpa_causal_strided

    hq, hkv, q_len, kv_len, d, dtype = case
    c = S.make_stair(*case)
    if not strided:
        out = _nan_out((hq, q_len, d), dtype)
        assert sdpa_causal(_dev(c.q, dtype), _dev(c.k, dtype), _dev(c.v, dtype), 1.0, out=out) is out
        return c, out
    q, k, v = (_dev(np.ascontiguousarray(a.transpose(1, 0, 2)), dtype) for a in (c.q, c.k, c.v))      # [S, H, D]
    out = _nan_out((q_len, hq, d), dtype)
    sdpa_causal_strided(q, k, v, out, hq, hkv, q_len, kv_len, d, (d, hq * d), (d, hkv * d), (d, hq * d), 1.0)
    return c, out


def _check_causal(case):
    c, out = _run_causal(case)
    _assert_rows(out, c.expected(case[3] - case[2]), case[5], _dense_v_rows(c))


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("case", S.FLASH2, ids=str)
def test_sdpa_causal_second_generation_flash(case, dtype):
    assert case[2] > 128
    _check_causal(case + (dtype,))


@pytest.mark.parametrize("case", S.ONE_TILE, ids=str)
def test_sdpa_causal_one_tile_kernel(case):
    assert case[2] <= 128 and case[3] <= 128 and case[4] == 128
    _check_causal(case + ("bf16",))


@pytest.mark.parametrize("case", S.GEN1, ids=str)
def test_sdpa_causal_first_generation_kernel(case):
    assert case[2] <= 128 and (case[3] > 128 or case[4] != 128 or case[5] != "bf16")
    _check_causal(case)


@pytest.mark.parametrize("case", S.NAIVE, ids=str)
def test_sdpa_causal_naive_fallback(case):
    assert case[5] == "f32" or case[4] not in (64, 128)
    _check_causal(case)


def test_sdpa_causal_naive_fallback_when_flash_attention_is_switched_off(monkeypatch):
    monkeypatch.setenv("PYGPUKIT_FLASH_ATTENTION", "0")
    _check_causal(S.NAIVE_ENV)


@pytest.mark.parametrize("case", [S.FLASH2[1] + ("bf16",), S.ONE_TILE[3] + ("bf16",), S.GEN1[0], S.NAIVE[0]], ids=str)
def test_sdpa_causal_strided_equals_the_contiguous_call(case):
    """[S,H,D] buffers, one case per kernel generation (flash, one-tile, first generation, fallback)."""
    hq, hkv, q_len, kv_len, d, dtype = case
    c, out = _run_causal(case, strided=True)
    got = _host(out, dtype).transpose(1, 0, 2)
    _, ref = _run_causal(case)
    np.testing.assert_array_equal(got, _host(ref, dtype))
    want = c.expected(kv_len - q_len)
    if dtype == "f32":
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=0.0)
    else:
        np.testing.assert_array_equal(got, S.to_words(want, dtype))


def test_sdpa_causal_long_prompt_on_the_first_generation_kernel():
    """Output rows that are no multiple of 8 bytes apart keep a q_len > 128 call off the second-generation kernel: the
    first-generation kernel then walks five 64-row query tiles per head."""
    from pygpukit_amd.ops.nn.attention import sdpa_causal_strided

    hq, hkv, q_len, kv_len, d, dtype = case = S.FLASH2[1] + ("bf16",)
    c = S.make_stair(*case)
    q, k, v = (_dev(np.ascontiguousarray(a.transpose(1, 0, 2)), dtype) for a in (c.q, c.k, c.v))      # [S, H, D]
    pitch = hq * d + 2
    out = _nan_out((q_len, pitch), dtype)
    sdpa_causal_strided(q, k, v, out, hq, hkv, q_len, kv_len, d, (d, hq * d), (d, hkv * d), (d, pitch), 1.0)
    got = _host(out, dtype)
    np.testing.assert_array_equal(got[:, hq * d:], NAN_WORD[dtype])                                  # the gap between rows is untouched
    rows = got[:, :hq * d].reshape(q_len, hq, d).transpose(1, 0, 2)
    want = S.to_words(c.expected(kv_len - q_len), dtype)
    np.testing.assert_array_equal(rows, want, err_msg="" if np.array_equal(rows, want) else _explain(rows, want, _dense_v_rows(c), dtype))


# ---- sdpa_causal_fp8 ---------------------------------------------------------------------------------------------------

def _needs_fp8():
    from pygpukit_amd.ops.nn.attention import fa3_fp8_available

    assert fa3_fp8_available(), "sdpa_causal_fp8 needs the gfx950 device these tests run on"


def _fp8_exact_rows(c: S.Stair, last_key: np.ndarray) -> np.ndarray:
    """Rows whose scores stay below 2**16 in the exp2 domain (512 units of headroom for the noise columns, whose sum has a
    standard deviation near 2), and a check that no score reaches 2**17: see test_sdpa_causal_fp8."""
    top = c.s * last_key * 1.4426950408889634
    assert top.max() + 512.0 < 131072.0
    return top + 512.0 < 65536.0


@pytest.mark.parametrize("case", S.FP8, ids=str)
def test_sdpa_causal_fp8(case):
    """Exact on every row whose last visible key lies below 704; ONE bf16 ulp on the rows beyond (only (2,1,130,1030,128) has
    any: its first run, bit-exact comparison on all rows, had 49 of 260 rows off by one ulp in 5.4 % of their elements).

    The reason is in flash_softmax_pv<.., SCALED = true> (csrc/flash_core.hip.h), the step flash_fwd_fp8_kernel
    (csrc/ops_flash_fp8.hip) runs on each tile.  The MFMA leaves RAW fp8 sums; the running maximum is
    `mx = max(raw) * cf`, one fp32 rounding of the product, and the probabilities are `exp2(fmaf(raw, cf, -m_use))`, the
    product NOT rounded before the subtraction.  For the key that holds the maximum the exponent is therefore the rounding
    error of raw * cf instead of 0 (flash_fwd_kernel, whose MFMA returns the scaled scores themselves, subtracts a score
    from itself).  Scores in [2**16, 2**17) have an fp32 ulp of 2**-7, so that exponent reaches +-2**-8 and the largest
    probability lies in 1 +- 0.0027.  The numerator then carries it rounded to bf16 (1.0 or 1 - 2**-8), the row sum carries
    it unrounded, and out = V * P / l is off by up to 0.0027 relative: above bf16's smallest relative half-ulp, 2**-9 =
    0.00195, and below three of them, hence at most one ulp.  Below 2**16 the ulp is 2**-8 or finer, the probability lies
    in 1 +- 0.00135, rounds to exactly 1.0 in bf16 and moves the quotient by less than any half-ulp: those rows are exact.
    A mask that is off by one key returns another V row, which is no closer than any two N(0,1) rows are."""
    from pygpukit_amd.ops.nn.attention import sdpa_causal_fp8

    _needs_fp8()
    hq, hkv, q_len, kv_len, d = case
    c = S.make_stair(*case, "bf16")
    out = _nan_out((hq, q_len, d), "bf16")
    sdpa_causal_fp8(_dev(c.q, "bf16"), _dev(c.k, "bf16"), _dev(c.v, "bf16"), out, 1.0)
    exact = _fp8_exact_rows(c, kv_len - q_len + np.arange(q_len))
    assert exact.all() or case == (2, 1, 130, 1030, 128)
    if exact.all():
        _assert_rows(out, c.expected(kv_len - q_len), "bf16", _dense_v_rows(c))
        return
    got, want = _host(out, "bf16"), S.to_words(c.expected(kv_len - q_len), "bf16")
    np.testing.assert_array_equal(got[:, exact], want[:, exact])
    ulps = np.abs(got.astype(np.int32) - want.astype(np.int32))        # same-sign bf16 words one apart are one ulp apart
    print(f"sdpa_causal_fp8 {case}: {int((ulps > 0).sum())} of {ulps.size} elements off by one ulp, max {int(ulps.max())}")
    far = np.where(ulps <= 1, got, want)                               # differs from `got` only where more than one ulp off
    assert ulps.max() <= 1, _explain(got, far, _dense_v_rows(c), "bf16")


def test_sdpa_causal_fp8_strided_equals_the_contiguous_call():
    from pygpukit_amd.ops.nn.attention import sdpa_causal_fp8, sdpa_causal_fp8_strided

    _needs_fp8()
    hq, hkv, q_len, kv_len, d = case = S.FP8[2]
    c = S.make_stair(*case, "bf16")
    q, k, v = (_dev(np.ascontiguousarray(a.transpose(1, 0, 2)), "bf16") for a in (c.q, c.k, c.v))
    out = _nan_out((q_len, hq, d), "bf16")
    sdpa_causal_fp8_strided(q, k, v, out, hq, hkv, q_len, kv_len, d, (d, hq * d), (d, hkv * d), (d, hq * d), 1.0)
    ref = _nan_out((hq, q_len, d), "bf16")
    sdpa_causal_fp8(_dev(c.q, "bf16"), _dev(c.k, "bf16"), _dev(c.v, "bf16"), ref, 1.0)
    got = _host(out, "bf16").transpose(1, 0, 2)
    np.testing.assert_array_equal(got, _host(ref, "bf16"))
    np.testing.assert_array_equal(got, S.to_words(c.expected(kv_len - q_len), "bf16"))


# ---- sdpa_irope --------------------------------------------------------------------------------------------------------

def _run_irope(case, offset, pos_dtype=np.int64):
    from pygpukit_amd.ops.nn.llama4 import sdpa_irope

    hq, hkv, q_len, kv_len, d, dtype, _ = case
    c = S.make_stair(hq, hkv, q_len, kv_len, d, dtype, S.irope_scale(d))
    pos = _raw((IROPE_START + np.arange(q_len)).astype(pos_dtype))
    out = sdpa_irope(_dev(c.q, dtype), _dev(c.k, dtype), _dev(c.v, dtype), pos, IROPE_ATTN_SCALE, IROPE_FLOOR_SCALE, offset)
    return c, out


@pytest.mark.parametrize("pos_dtype", [np.int64, np.int32], ids=["i64", "i32"])
@pytest.mark.parametrize("case", S.IROPE, ids=str)
def test_sdpa_irope_full_offset(case, pos_dtype):
    off = case[3] - case[2]
    c, out = _run_irope(case, off, pos_dtype)
    _assert_rows(out, c.expected(off), case[5], _dense_v_rows(c))


@pytest.mark.parametrize("case", [t for t in S.IROPE if t[6] is not None], ids=str)
def test_sdpa_irope_smaller_offset_moves_the_expected_rows(case):
    """kv_seen = offset + q_len < kv_len: the keys beyond it (the highest stairs) must stay unseen."""
    c, out = _run_irope(case, case[6])
    _assert_rows(out, c.expected(case[6]), case[5], _dense_v_rows(c))


@pytest.mark.parametrize("case", [t for t in S.IROPE if t[6] is not None], ids=str)
def test_sdpa_irope_offset_plus_one_returns_exactly_the_next_rows(case):
    """Sensitivity on the device: causal_offset + 1 returns the next V row on every row (all have one here)."""
    c, out = _run_irope(case, case[6] + 1, np.int32)
    got = _assert_rows(out, c.expected(case[6] + 1), case[5], _dense_v_rows(c))
    assert (got != S.to_words(c.expected(case[6]), case[5])).any(axis=2).all()


# ---- sdpa_alibi --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", S.ALIBI, ids=str)
def test_sdpa_alibi(case):
    from pygpukit_amd.ops.nn.alibi import sdpa_alibi

    hq, hkv, q_len, kv_len, d, dtype = case
    c = S.make_stair(*case)
    out = _nan_out((hq, q_len, d), dtype)
    sdpa_alibi(_dev(c.q, dtype), _dev(c.k, dtype), _dev(c.v, dtype), _raw(S.alibi_slopes(hq)), 1.0, out=out)
    _assert_rows(out, c.expected(kv_len - q_len), dtype, _dense_v_rows(c))


# ---- fixed-cache decode ------------------------------------------------------------------------------------------------
# The caches are filled along their whole length: rows at or past context_len carry the HIGHEST stairs, so an over-read
# by one row wins the softmax.

def _i32(v):
    return _raw(np.array([v], np.int32))


def _cache_case(op, hq, hc, d, dtype, max_seq, q_len=1):
    return S.make_stair(hq, hc, q_len, max_seq, d, dtype, S.irope_scale(d) if op == "irope" else 1.0)


def _run_fixed_cache(op, c: S.Stair, ctx, ptr=False):
    from pygpukit_amd.ops.nn import alibi, attention, llama4

    hq, _, q_len, max_seq, d = c.shape
    dt = c.dtype
    q, k, v, out = _dev(c.q, dt), _dev(c.k, dt), _dev(c.v, dt), _nan_out((hq, q_len, d), dt)
    if op == "causal":
        if ptr:
            attention.sdpa_causal_fixed_cache_ptr(q, k, v, out, _i32(ctx), max_seq, 1.0)
        else:
            attention.sdpa_causal_fixed_cache(q, k, v, out, ctx, 1.0)
    elif op == "alibi":
        sl = _raw(S.alibi_slopes(hq))
        if ptr:
            alibi.sdpa_alibi_fixed_cache_ptr(q, k, v, sl, out, _i32(ctx), max_seq, 1.0)
        else:
            alibi.sdpa_alibi_fixed_cache(q, k, v, sl, out, ctx, 1.0)
    else:
        if ptr:
            llama4.sdpa_irope_fixed_cache_ptr(q, k, v, out, _i32(ctx - 1), IROPE_ATTN_SCALE, IROPE_FLOOR_SCALE)
        else:
            llama4.sdpa_irope_fixed_cache(q, k, v, out, ctx - 1, IROPE_ATTN_SCALE, IROPE_FLOOR_SCALE)
    return out


def _check_fixed_cache(op, hq, hc, d, dtype, max_seq, ctx, q_len=1, ptr=False):
    c = _cache_case(op, hq, hc, d, dtype, max_seq, q_len)
    out = _run_fixed_cache(op, c, ctx, ptr)
    return _assert_rows(out, c.expected(ctx - q_len), dtype, _dense_v_rows(c))


@pytest.mark.parametrize("max_seq,ctx", S.DECODE_CTX)
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("hq,hc", S.DECODE_HEADS)
def test_sdpa_causal_fixed_cache(hq, hc, d, dtype, max_seq, ctx):
    _check_fixed_cache("causal", hq, hc, d, dtype, max_seq, ctx)


@pytest.mark.parametrize("max_seq,ctx", S.DECODE_CTX)
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("hq,hc", S.DECODE_HEADS)
@pytest.mark.parametrize("op", ["alibi", "irope"])
def test_sdpa_alibi_and_irope_fixed_cache(op, hq, hc, d, max_seq, ctx):
    _check_fixed_cache(op, hq, hc, d, "bf16", max_seq, ctx)


@pytest.mark.parametrize("max_seq,ctx", S.DECODE_CTX)
@pytest.mark.parametrize("hq,hc,d", [(4, 2, 128), (5, 1, 64)])
@pytest.mark.parametrize("op", ["causal", "alibi", "irope"])
def test_fixed_cache_ptr_form_equals_the_host_form_bit_for_bit(op, hq, hc, d, max_seq, ctx):
    c = _cache_case(op, hq, hc, d, "bf16", max_seq)
    host = _host(_run_fixed_cache(op, c, ctx), "bf16")
    got = _check_fixed_cache(op, hq, hc, d, "bf16", max_seq, ctx, ptr=True)
    np.testing.assert_array_equal(got, host)


@pytest.mark.parametrize("op", ["alibi", "irope"])
def test_fixed_cache_five_heads_per_workgroup(op):
    hq, hkv, max_seq, d = S.DECODE_G5
    _check_fixed_cache(op, hq, hkv, d, "bf16", max_seq, 1500)


@pytest.mark.parametrize("op,d,dtype", [("causal", 128, "bf16"), ("causal", 64, "bf16"), ("causal", 128, "f32"), ("alibi", 128, "bf16")])
def test_fixed_cache_five_query_rows_take_the_general_path(op, d, dtype):
    """q_len 5 at context 75: the prefill kernels over the cache prefix in place (one-tile, first generation, fallback;
    the flash kernel for ALiBi)."""
    _check_fixed_cache(op, 4, 2, d, dtype, 1024, 75, q_len=5)


@pytest.mark.parametrize("ctx", [100, 257])
def test_sdpa_causal_fixed_cache_with_flash_decoding_switched_off(monkeypatch, ctx):
    """One query row through the prefill kernels (one-tile at 100 cached rows, first generation at 257)."""
    monkeypatch.setenv("PYGPUKIT_FLASH_DECODING", "0")
    _check_fixed_cache("causal", 4, 2, 128, "bf16", 1024, ctx)


# ---- paged_attention_v1 ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("cfg", S.PAGED, ids=str)
def test_paged_attention_v1(cfg, dtype):
    """Scattered pages; page 0, unreferenced pages and the tail slots of every last page hold stairs above every valid key."""
    from pygpukit_amd.ops.paged import paged_attention_v1

    num_seqs, hq, hkv, d, bs, ctxs = cfg
    p = S.make_paged(*cfg, dtype)
    out = _nan_out((num_seqs, hq, d), dtype)
    paged_attention_v1(_dev(p.q, dtype), _dev(p.k, dtype), _dev(p.v, dtype), _raw(p.tables), _raw(p.ctxs), 1.0, out=out,
                       max_context=max(ctxs))
    vw = S.to_words(p.v, dtype)                                            # [blocks, hkv, bs, d]
    _assert_rows(out, p.expected, dtype, lambda idx: vw[:, idx[1] // (hq // hkv)].reshape(-1, d))
