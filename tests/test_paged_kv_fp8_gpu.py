"""FP8 (e4m3) paged KV cache on the GPU: the page writer byte for byte against tests/kv_fp8_ref.py; decode and packed prefill against
the float64 oracle (tests/paged_prefill_ref.py on the caches dequantised by kv_fp8_ref.dequantise: the SAME CODES the kernels read, so
the bar measures the kernels, not the quantisation); exact checks of the scales and the mask.  Bar: rel_err <= 1e-2 and an all-finite
output, as test_kv_fp8_gpu.py and test_paged_prefill_gpu.py.  Every byte of both caches outside the live rows is the NaN code 0x7F
and the pages are a random permutation: a wrong page, a row fetched past ctx or a multiply-by-zero mask shows as a non-finite output."""

import functools

import numpy as np
import pytest

from tests import attn_stair_ref as S
from tests import kv_fp8_ref as R
from tests import paged_prefill_ref as P
from tests.conftest import rel_err
from tests.test_kv_fp8_gpu import W_SCALES, _writer_input
from tests.test_paged_prefill_gpu import BLIND, MIXED

pytestmark = pytest.mark.gpu

NAN_CODE, SENTINEL, PAD_ROWS = 0x7F, 0x4A4A, 3
CASES = [pytest.param(dtype, d, heads, bs, id=f"{dtype}-D{d}-H{heads[0]}x{heads[1]}-bs{bs}")
         for dtype in ("bf16", "f16") for d in (64, 128) for heads in ((4, 2), (8, 1), (2, 2)) for bs in (8, 48, 128)]
params = pytest.mark.parametrize("dtype,d,heads,bs", CASES)


def _up(*arrays):
    from pygpukit_amd.core import from_numpy

    return [from_numpy(np.ascontiguousarray(a)) for a in arrays]


def _dev(x, dtype, words=False):
    w = x if words else S.to_words(x, dtype)
    return _up(w.view(np.float16) if dtype == "f16" else w)[0]


def _words(a):
    return a.to_numpy().view(np.uint16)


def _tables(rng, ctxs, bs):
    """-> block_tables, num_blocks: a random permutation of the pages; five stay unused, the unused table entries point at one"""
    need = -(-np.asarray(ctxs) // bs)
    num_blocks = int(need.sum()) + 5
    pages = rng.permutation(num_blocks)
    slots = [(b, j) for b in range(len(ctxs)) for j in range(need[b])]
    tables = np.full((len(ctxs), int(need.max()) + 1), pages[-1], np.int32)
    for (b, j), page in zip([slots[i] for i in rng.permutation(len(slots))], pages):
        tables[b, j] = page
    return tables, num_blocks


def _place(cache, tables, b, rows):
    pos = np.arange(len(rows))                  # rows [ctx, Hkv, D] of sequence b -> its pages
    cache[tables[b][pos // cache.shape[2]], :, pos % cache.shape[2]] = rows


@functools.lru_cache(maxsize=None)
def _case(pairs, dtype, d, heads, bs):
    hq, hkv = heads
    rng = np.random.default_rng(hq * 100 + hkv * 10 + d + bs + len(pairs))
    ctxs = np.array([p[1] for p in pairs], np.int32)
    cu = np.concatenate([[0], np.cumsum([p[0] for p in pairs])]).astype(np.int32)
    tables, num_blocks = _tables(rng, ctxs, bs)
    q = S.round_to(rng.standard_normal((int(cu[-1]) + PAD_ROWS, hq, d)), dtype)
    ks, vs = (rng.uniform(0.005, 0.02, hkv).astype(np.float32) for _ in range(2))       # ~ absmax / 224 of a unit normal
    kc, vc = (np.full((num_blocks, hkv, bs, d), NAN_CODE, np.uint8) for _ in range(2))
    for b, ctx in enumerate(ctxs):
        for cache, sc in ((kc, ks), (vc, vs)):
            _place(cache, tables, b, R.quantise(rng.standard_normal((ctx, hkv, d)), sc))
    ref = P.paged_attention_prefill(q, R.dequantise(kc, ks, head_axis=1), R.dequantise(vc, vs, head_axis=1), tables, ctxs, cu)
    return q, kc, vc, ks, vs, tables, ctxs, cu, ref


def _run(op, case, dtype, **kw):
    from pygpukit_amd.ops import paged

    q, kc, vc, ks, vs, tables, ctxs, cu, _ = case
    rows = q[:len(ctxs)] if op == "decode" else q
    out = _dev(np.full(rows.shape, SENTINEL, np.uint16), dtype, words=True)
    fn, extra = (paged.paged_attention_v1_fp8, ()) if op == "decode" else (paged.paged_attention_prefill_fp8, (cu,))
    fn(_dev(rows, dtype), *_up(kc, vc, ks, vs, tables, ctxs, *extra), out=out, **kw)
    return _words(out)


def _check(name, words, ref, dtype):
    got = S.from_words(words, dtype).astype(np.float64)
    e = rel_err(got, ref)
    print(f"{name}: rel_err {e:.3e}")
    assert np.isfinite(got).all() and e <= 1e-2, f"{name}: rel_err {e:.3e}"


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("bs", [8, 48, 128])
def test_writer_bytes(bs, d, dtype):
    from pygpukit_amd.ops.paged import reshape_and_cache_fp8

    tokens, num_blocks, fill = 37, 6, 0xA5
    x = {"k": _writer_input(tokens, d, dtype), "v": _writer_input(tokens, d, dtype)[::-1].copy()}       # V: the same rows, last first
    scales = {"k": W_SCALES, "v": W_SCALES[::-1].copy()}
    slots = np.random.default_rng(bs + d).permutation(num_blocks * bs)[:tokens].astype(np.int32)
    slots[11], live = -1, np.arange(tokens) != 11
    want = {n: np.full((num_blocks, 2, bs, d), fill, np.uint8) for n in x}
    for n in x:
        want[n][slots[live] // bs, :, slots[live] % bs] = R.quantise(x[n], scales[n])[live]
        assert (want[n] == 0x7E).any() and (want[n] == 0x80).any()
    kc, vc = _up(*(np.full((num_blocks, 2, bs, d), fill, np.uint8) for _ in range(2)))
    reshape_and_cache_fp8(_dev(x["k"], dtype), _dev(x["v"], dtype), kc, vc, *_up(slots, scales["k"], scales["v"]))
    for n, cache in (("k", kc), ("v", vc)):
        got = cache.to_numpy()
        np.testing.assert_array_equal(got, want[n], err_msg=n)      # the codes where they belong, the fill everywhere else
        assert not np.isin(got, (0x7F, 0xFF)).any()


@params
def test_decode_against_the_oracle(dtype, d, heads, bs):
    step = 32 if d == 128 else 64
    long_ctxs = (0, 1, step - 1, step, step + 1, bs - 1, bs + 1, 511, 512, 513, 1100)
    for ctxs, max_context in ((long_ctxs, 1100), ((0, 1, step + 1, bs + 1, 300, 512), 512)):         # three slices, then one
        case = _case(tuple((1, c) for c in ctxs), dtype, d, heads, bs)
        words = _run("decode", case, dtype, max_context=max_context)
        _check(f"paged_attention_v1_fp8 {dtype} D {d} heads {heads} block {bs} bound {max_context}", words, case[8][:len(ctxs)], dtype)
        assert (words[0] == 0).all()                                # ctx = 0: zeros, not the sentinel


@params
def test_prefill_against_the_oracle(dtype, d, heads, bs):
    case = _case(MIXED + BLIND, dtype, d, heads, bs)
    cu, ref = case[7], case[8]
    words = _run("prefill", case, dtype)
    _check(f"paged_attention_prefill_fp8 {dtype} D {d} heads {heads} block {bs}", words[:cu[-1]], ref[:cu[-1]], dtype)
    assert (words[cu[-1]:] == SENTINEL).all() and (words[cu[-2]:cu[-2] + 4] == 0).all()     # unowned rows untouched; blind rows zeros
    np.testing.assert_array_equal(_run("prefill", case, dtype, max_query_len=130), words)      # the early-exit workgroups change nothing


@params
def test_scales_and_mask_exactly(dtype, d, heads, bs):
    """K codes 0: uniform softmax over 256 rows; V[r, h, j] = 4 where (r + j + h) % 8 <= j % 8, else 0: mean (j % 8 + 1) / 2, exactly."""
    from pygpukit_amd.ops.paged import paged_attention_prefill_fp8, paged_attention_v1_fp8

    (hq, hkv), ctx = heads, 256
    rng = np.random.default_rng(d + bs)
    tables, num_blocks = _tables(rng, [ctx], bs)
    r, h, j = np.ogrid[:ctx, :hkv, :d]
    kc, vc = (np.full((num_blocks, hkv, bs, d), NAN_CODE, np.uint8) for _ in range(2))
    _place(kc, tables, 0, np.zeros((ctx, hkv, d), np.uint8))
    _place(vc, tables, 0, R.quantise(np.where((r + j + h) % 8 <= j % 8, 4.0, 0.0), np.ones(hkv)))
    mean = np.broadcast_to((np.arange(d) % 8 + 1) / 2.0, (1, hq, d))
    q = _dev(rng.standard_normal((1, hq, d)), dtype)
    kd, vd, td, cd, cud = _up(kc, vc, tables, np.array([ctx], np.int32), np.array([0, 1], np.int32))
    for k_scale, v_scale in ((1.0, 0.5), (3.7, 0.5), (1.0, 1.0)):
        ksd, vsd = _up(np.full(hkv, k_scale, np.float32), np.full(hkv, v_scale, np.float32))
        dec = paged_attention_v1_fp8(q, kd, vd, ksd, vsd, td, cd, max_context=1100)          # three slices
        pre = paged_attention_prefill_fp8(q, kd, vd, ksd, vsd, td, cd, cud)
        for name, out in (("decode", dec), ("prefill", pre)):
            np.testing.assert_array_equal(S.from_words(_words(out), dtype), mean * v_scale, err_msg=f"{name}, scales {k_scale} / {v_scale}")


def test_round_trip_through_the_public_ops():
    from pygpukit_amd.core.dtypes import uint8
    from pygpukit_amd.ops.paged import allocate_kv_cache, paged_attention_prefill_fp8, reshape_and_cache_fp8

    dtype, tokens, hq, hkv, d, bs = "bf16", 70, 4, 2, 64, 16
    rng = np.random.default_rng(70)
    tables, num_blocks = _tables(rng, [tokens], bs)
    q, k, v = (S.round_to(rng.standard_normal((tokens, h, d)) * g, dtype) for h, g in ((hq, 1.0), (hkv, 2.0), (hkv, 0.5)))
    ks, vs = R.absmax_scales(k), R.absmax_scales(v)
    slots = (tables[0][np.arange(tokens) // bs] * bs + np.arange(tokens) % bs).astype(np.int32)
    kc, vc = (allocate_kv_cache(num_blocks, hkv, bs, d, uint8) for _ in range(2))
    ksd, vsd, td, cd, cud = _up(ks, vs, tables, np.array([tokens], np.int32), np.array([0, tokens], np.int32))
    reshape_and_cache_fp8(_dev(k, dtype), _dev(v, dtype), kc, vc, _up(slots)[0], ksd, vsd)
    out = paged_attention_prefill_fp8(_dev(q, dtype), kc, vc, ksd, vsd, td, cd, cud)
    want = [np.zeros((num_blocks, hkv, bs, d), np.uint8) for _ in range(2)]
    for cache, x, sc in zip(want, (k, v), (ks, vs)):
        _place(cache, tables, 0, R.quantise(x, sc))
    ref = P.paged_attention_prefill(q, R.dequantise(want[0], ks, head_axis=1), R.dequantise(want[1], vs, head_axis=1), tables, [tokens], [0, tokens])
    _check("round trip", _words(out), ref, dtype)
