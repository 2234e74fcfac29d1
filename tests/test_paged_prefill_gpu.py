"""paged_attention_prefill on the GPU: one mixed packed batch against the float64 oracle (tests/paged_prefill_ref.py) on the
rounded inputs, exact 16-bit words where the result is one V row or zeros, and the grid bound.

Bar: rel_err <= 1e-2 and an all-finite output, what every 16-bit sdpa_* parity test here holds.  Every element of both caches
is NaN before the live rows are written, so a wrong page, a row past ctx or a multiply-by-zero mask shows as a non-finite output."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from tests import attn_stair_ref as S
from tests import paged_prefill_ref as P
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu

# (q_len, ctx): smallest decode row | decode row among prompts | idle | one ragged tile | exactly a tile | one row past a tile |
# a second column tile at G = 1 and a ragged key tile | chunk after a long prefix | chunk after a prefix, ctx no tile multiple
MIXED = ((1, 1), (1, 200), (0, 37), (33, 33), (64, 64), (65, 65), (130, 130), (5, 300), (128, 257))
BLIND = ((8, 4),)               # rows 0-3 fall before position 0 and see nothing
PAD_ROWS, SENTINEL = 3, 0x4A4A  # rows of out past cu[-1]; the word they are pre-filled with
NAN_WORD = {"bf16": 0x7FC0, "f16": 0x7E00}
CASES = [pytest.param(dtype, d, heads, bs, id=f"{dtype}-D{d}-H{heads[0]}x{heads[1]}-bs{bs}")
         for dtype in ("bf16", "f16") for d in (64, 128) for heads in ((4, 2), (8, 1), (2, 2)) for bs in (16, 48, 128)]
params = pytest.mark.parametrize("dtype,d,heads,bs", CASES)


@functools.lru_cache(maxsize=None)
def _case(pairs, dtype, d, heads, bs):
    """Inputs as float32 values of `dtype` (caches NaN outside the live rows), tables, lengths, and the oracle's output."""
    hq, hkv = heads
    rng = np.random.default_rng(hq * 100 + hkv * 10 + d + bs + len(pairs))
    q_lens, ctxs = np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)
    cu = np.concatenate([[0], np.cumsum(q_lens)]).astype(np.int32)
    need = -(-ctxs // bs)
    num_blocks, max_blocks = int(need.sum()) + 5, int(need.max()) + 1
    # physical pages: a random permutation dealt to the (sequence, logical block) slots in random order; five stay unused, and the
    # unused table entries point at one of those
    pages = rng.permutation(num_blocks)
    slots = [(b, j) for b in range(len(pairs)) for j in range(need[b])]
    tables = np.full((len(pairs), max_blocks), pages[-1], np.int32)
    for (b, j), page in zip([slots[i] for i in rng.permutation(len(slots))], pages):
        tables[b, j] = page
    q = S.round_to(rng.standard_normal((int(cu[-1]) + PAD_ROWS, hq, d)), dtype)
    kc, vc = (np.full((num_blocks, hkv, bs, d), np.nan, np.float32) for _ in range(2))
    for b, ctx in enumerate(ctxs):
        pos = np.arange(ctx)
        for cache in (kc, vc):
            cache[tables[b][pos // bs], :, pos % bs] = S.round_to(rng.standard_normal((ctx, hkv, d)), dtype)
    ref = P.paged_attention_prefill(q, kc, vc, tables, ctxs, cu)
    for a in (q, kc, vc, tables, ctxs, cu, ref):
        a.setflags(write=False)
    return q, kc, vc, tables, ctxs, cu, ref


def _dev(x, dtype):
    from pygpukit_amd.core import from_numpy

    w = np.where(np.isnan(x), np.uint16(NAN_WORD[dtype]), S.to_words(np.nan_to_num(x), dtype))
    return from_numpy(np.ascontiguousarray(w.view(np.float16) if dtype == "f16" else w))


def _run(case, dtype, **kw):
    """-> the output's 16-bit words [total_tokens, Hq, D]"""
    from pygpukit_amd.core import from_numpy
    from pygpukit_amd.ops.paged import paged_attention_prefill

    q, kc, vc, tables, ctxs, cu, _ = case
    out = from_numpy(np.full(q.shape, SENTINEL, np.uint16).view(np.float16 if dtype == "f16" else np.uint16))
    got = paged_attention_prefill(_dev(q, dtype), _dev(kc, dtype), _dev(vc, dtype), from_numpy(tables), from_numpy(ctxs), from_numpy(cu), out=out, **kw)
    h = got.to_numpy()
    return h if h.dtype == np.uint16 else h.view(np.uint16)


@params
def test_mixed_batch_against_the_oracle(dtype, d, heads, bs):
    case = _case(MIXED, dtype, d, heads, bs)
    cu, ref = case[5], case[6]
    words = _run(case, dtype)
    got = S.from_words(words[:cu[-1]], dtype).astype(np.float64)
    e = rel_err(got, ref[:cu[-1]])
    print(f"paged_attention_prefill {dtype} D {d} heads {heads} block {bs}: rel_err {e:.3e}")
    assert np.isfinite(got).all() and e <= 1e-2
    assert (words[cu[-1]:] == SENTINEL).all()          # rows no sequence owns are not touched


@params
def test_rows_of_one_key_and_of_none_are_exact_words(dtype, d, heads, bs):
    rep = heads[0] // heads[1]
    q, kc, vc, tables, ctxs, cu, _ = case = _case(MIXED, dtype, d, heads, bs)
    words = _run(case, dtype)
    for b, (q_len, ctx) in enumerate(MIXED):
        if q_len and q_len == ctx:      # local row 0 sees key 0 alone: V row 0 of its kv head, bit for bit
            v0 = P.gather(vc, tables[b], 1)[:, 0]
            np.testing.assert_array_equal(words[cu[b]], S.to_words(v0[np.arange(heads[0]) // rep], dtype), err_msg=f"sequence {b}")
    q, kc, vc, tables, ctxs, cu, _ = case = _case(BLIND, dtype, d, heads, bs)
    words = _run(case, dtype)
    assert (words[:4] == 0).all()
    np.testing.assert_array_equal(words[4], S.to_words(P.gather(vc, tables[0], 1)[:, 0][np.arange(heads[0]) // rep], dtype))


@params
def test_tight_and_default_max_query_len_agree(dtype, d, heads, bs):
    """max_query_len = 130 (the longest run) and the default (total_tokens): the early-exit workgroups change nothing."""
    case = _case(MIXED, dtype, d, heads, bs)
    np.testing.assert_array_equal(_run(case, dtype, max_query_len=130), _run(case, dtype))
