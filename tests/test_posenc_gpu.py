"""GPU tests of the positional-encoding family: uploaded tables, pope_inplace, alibi_compute_bias, alibi_add_bias, and ALiBi
inside attention (sdpa_alibi on the flash-prefill kernel, sdpa_alibi_fixed_cache on the split-KV decode walk).

Bars.  Tables, slopes, PoPE, bias and add_bias are bit-exact against the reference's CPU path (tests/golden/g8_posenc.npz)
and the NumPy restatement (tests/posenc_ref.py).  Attention: rel_err <= 1e-2 against the fp64 restatement on 16-bit-rounded
inputs - the project's bf16 bar, which sdpa_causal and sdpa_irope meet with the same kernels; the bias is fp32 arithmetic
added to fp32 scores and brings no new rounding.  Without the bias (or with the slopes reversed) the result is more than
1e-1 away from the oracle on these cases, so the bar separates "applied" from "not applied" by a factor of ten."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from oracle import cpu_ref as O
from tests import posenc_ref as P
from tests.conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

BAR = 1e-2
FAR = 1e-1
MAX_SEQ = 1024          # 4 KV splits
NAN_BITS = {"bf16": 0x7FC0, "f16": 0x7E00}
TABLE_SHAPES = ((64, 16, 10000.0), (70, 40, 500000.0), (300, 128, 10000.0))


@functools.lru_cache(maxsize=None)
def _g():
    return load_golden("g8_posenc.npz")


def _bits(x, dtype) -> np.ndarray:
    """float32 values -> the 16-bit words of `dtype`."""
    x = np.ascontiguousarray(x, np.float32)
    return O.f32_to_bf16_bits(x) if dtype == "bf16" else x.astype(np.float16).view(np.uint16)


def _dev_bits(words, dtype):
    from pygpukit_amd.core import from_numpy

    words = np.ascontiguousarray(words, np.uint16)
    return from_numpy(words if dtype == "bf16" else words.view(np.float16))


def _host_bits(a) -> np.ndarray:
    h = a.to_numpy()
    return h if h.dtype == np.uint16 else h.view(np.uint16)


def _values(words, dtype) -> np.ndarray:
    return O.bf16_bits_to_f32(words) if dtype == "bf16" else words.view(np.float16).astype(np.float32)


def _nan_out(shape, dtype):
    return _dev_bits(np.full(shape, NAN_BITS[dtype], np.uint16), dtype)


def _dev(a):
    from pygpukit_amd.core import from_numpy

    return from_numpy(np.ascontiguousarray(a))


def _i32(v):
    return _dev(np.array([v], np.int32))


# ---- tables and slopes -------------------------------------------------------------------------------------------------

def test_uploaded_tables_and_slopes_equal_the_reference():
    from pygpukit_amd.ops.nn import alibi_init_slopes, pope_init_encoding, rope_init_linear, rope_init_ntk_aware, rope_init_yarn

    g = _g()
    orig = int(g["yarn_original_max_len"])
    for S, D, base in TABLE_SHAPES:
        rows = g[f"rows_{S}"]
        for scale in (1.0, 2.0, 4.0):
            tag = f"{S}_{D}_{int(scale)}"
            for kind, tables in (("ntk", rope_init_ntk_aware(S, D, base, scale)), ("linear", rope_init_linear(S, D, base, scale)),
                                 ("yarn", rope_init_yarn(S, D, base, scale, original_max_len=orig, mscale=0.0))):
                for t, name in zip(tables, ("cos", "sin")):
                    h = t.to_numpy()
                    assert h.dtype == np.float32 and h.shape == (S, D)
                    np.testing.assert_array_equal(h[rows], g[f"{kind}_{name}_{tag}"], err_msg=f"{kind} {name} {tag}")
    cos, _ = rope_init_yarn(70, 40, 500000.0, 4.0, original_max_len=orig)                       # default mscale 0.1
    np.testing.assert_array_equal(cos.to_numpy(), P.rope_init_yarn(70, 40, 500000.0, 4.0, original_max_len=orig)[0])
    cos, sin = rope_init_linear(70, 40, 500000.0, 1.0, layout="half")
    want = O.precompute_freqs_cis(40, 70, 500000.0)
    np.testing.assert_array_equal(cos.to_numpy(), want[0])
    np.testing.assert_array_equal(sin.to_numpy(), want[1])
    np.testing.assert_array_equal(pope_init_encoding(16, 8).to_numpy(), g["pope_enc_16_8"])
    np.testing.assert_array_equal(pope_init_encoding(300, 128).to_numpy()[g["rows_300"]], g["pope_enc_300_128"])
    for h in (1, 2, 8, 12, 32, 40):
        np.testing.assert_array_equal(alibi_init_slopes(h).to_numpy(), g[f"slopes_{h}"])


# ---- pope_inplace ------------------------------------------------------------------------------------------------------

def test_pope_inplace_float32_equals_the_reference():
    from pygpukit_amd.ops.nn import pope_init_encoding, pope_inplace

    g = _g()
    q, k = _dev(g["pope_q"]), _dev(g["pope_k"])
    pope_inplace(q, k, pope_init_encoding(16, 8), start_pos=2)
    np.testing.assert_array_equal(q.to_numpy(), g["pope_q_y"])
    np.testing.assert_array_equal(k.to_numpy(), g["pope_k_y"])


@pytest.mark.parametrize("dtype,S,hq,hk,D,start", [("bf16", 130, 3, 1, 128, 7), ("f16", 130, 3, 1, 128, 7), ("f16", 40, 2, 2, 20, 3)])
def test_pope_inplace_16_bit_is_one_add_and_one_rounding(dtype, S, hq, hk, D, start):
    """D = 128 takes the 16-byte path, D = 20 the element-wise one."""
    from pygpukit_amd.ops.nn import pope_inplace

    rng = np.random.default_rng(S + D)
    qw, kw = _bits(rng.standard_normal((S, hq, D)), dtype), _bits(rng.standard_normal((S, hk, D)), dtype)
    enc = P.pope_init_encoding(S + start + 5, D)
    want_q, want_k = P.pope_inplace(_values(qw, dtype), _values(kw, dtype), enc, start, dtype)
    q, k = _dev_bits(qw, dtype), _dev_bits(kw, dtype)
    pope_inplace(q, k, _dev(enc), start_pos=start)
    np.testing.assert_array_equal(_host_bits(q), _bits(want_q, dtype))
    np.testing.assert_array_equal(_host_bits(k), _bits(want_k, dtype))
    assert (_host_bits(q) != qw).any() and (_host_bits(k) != kw).any()


# ---- alibi_compute_bias / alibi_add_bias -------------------------------------------------------------------------------

def test_alibi_compute_bias_equals_the_reference_and_the_restatement():
    from pygpukit_amd.ops.nn import alibi_compute_bias, alibi_init_slopes

    g = _g()
    s8 = alibi_init_slopes(8)
    np.testing.assert_array_equal(alibi_compute_bias(5, 8, s8).to_numpy(), g["bias_5_8_causal"])
    np.testing.assert_array_equal(alibi_compute_bias(5, 8, s8, causal=False).to_numpy(), g["bias_5_8_full"])
    slopes = np.array([0.3, 1e-4, 0.7071], np.float32)          # products that round
    for causal in (True, False):
        got = alibi_compute_bias(70, 3, _dev(slopes), causal=causal).to_numpy()
        assert got.shape == (3, 70, 70)
        np.testing.assert_array_equal(got, P.alibi_compute_bias(70, 3, slopes, causal))


def test_alibi_add_bias_equals_the_reference_exactly():
    """Equal, not close: a fused multiply-add would differ in the last bit of some elements."""
    from pygpukit_amd.ops.nn import alibi_add_bias

    g = _g()
    scores = _dev(g["add_bias_scores"])
    alibi_add_bias(scores, _dev(g["slopes_8"]), start_pos=4)
    np.testing.assert_array_equal(scores.to_numpy(), g["add_bias_y"])
    # slopes that are no powers of two: the product rounds, and a fused multiply-add gives other bits
    slopes = np.array([0.3, 1e-4, 0.7071, 0.11, 0.013, 0.9, 0.77, 0.05], np.float32)
    rng = np.random.default_rng(5)
    s2 = rng.standard_normal((2, 8, 3, 9)).astype(np.float32)
    want = P.alibi_add_bias(s2, slopes, 4)
    fused = (s2.astype(np.float64) - slopes.astype(np.float64)[None, :, None, None] * (4 + np.arange(3)[:, None] - np.arange(9)[None, :])).astype(np.float32)
    assert (want != fused).any()          # the case tells the two apart
    d = _dev(s2)
    alibi_add_bias(d, _dev(slopes), start_pos=4)
    np.testing.assert_array_equal(d.to_numpy(), want)


# ---- sdpa_alibi --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _qkv(hq, hkv, q_len, kv_len, d, dtype):
    rng = np.random.default_rng(1000 * q_len + kv_len + d)
    q, k, v = (_bits(rng.standard_normal(s).astype(np.float32), dtype) for s in ((hq, q_len, d), (hkv, kv_len, d), (hkv, kv_len, d)))
    for a in (q, k, v):
        a.setflags(write=False)
    return q, k, v


@functools.lru_cache(maxsize=None)
def _oracle(hq, hkv, q_len, kv_len, d, dtype, slopes: tuple):
    q, k, v = (_values(a, dtype) for a in _qkv(hq, hkv, q_len, kv_len, d, dtype))
    want = P.sdpa_alibi(q, k, v, np.array(slopes, np.float32))
    want.setflags(write=False)
    return want


def _run(hq, hkv, q_len, kv_len, d, dtype, slopes):
    from pygpukit_amd.ops.nn import sdpa_alibi

    q, k, v = (_dev_bits(a, dtype) for a in _qkv(hq, hkv, q_len, kv_len, d, dtype))
    out = _nan_out((hq, q_len, d), dtype)           # NaN everywhere: every element must be written
    got = sdpa_alibi(q, k, v, _dev(np.asarray(slopes, np.float32)), out=out)
    assert got is out
    vals = _values(_host_bits(out), dtype)
    assert np.isfinite(vals).all()
    return vals


def _std_slopes(hq) -> tuple:
    return tuple(P.alibi_init_slopes(hq).tolist())


CASES = [(4, 4, 200, 200, 128, "bf16"),        # partial tiles
         (8, 2, 129, 333, 128, "bf16"),        # GQA, prefix, one-row second tile
         (2, 2, 1, 70, 128, "bf16"),           # a decode row through the prefill kernel
         (2, 1, 512, 512, 128, "bf16"),        # two KV runs
         (2, 1, 600, 1100, 128, "bf16"),       # four runs and merge
         (4, 2, 200, 200, 64, "f16")]


@pytest.mark.parametrize("hq,hkv,q_len,kv_len,d,dtype", CASES)
def test_sdpa_alibi_matches_the_restatement(hq, hkv, q_len, kv_len, d, dtype):
    slopes = _std_slopes(hq)
    got = _run(hq, hkv, q_len, kv_len, d, dtype, slopes)
    err = rel_err(got, _oracle(hq, hkv, q_len, kv_len, d, dtype, slopes))
    print(f"sdpa_alibi ({hq},{hkv}) q {q_len} kv {kv_len} D {d} {dtype}: rel_err {err:.3e}")
    assert err <= BAR


def test_sdpa_alibi_steep_zero_and_flat_heads():
    from pygpukit_amd.ops.nn import sdpa_causal

    slopes = (2.0, 0.0, 0.3, 1e-4)
    case = (4, 4, 200, 200, 128, "bf16")
    got, want = _run(*case, slopes), _oracle(*case, slopes)
    for h in range(4):
        err = rel_err(got[h], want[h])
        print(f"sdpa_alibi slope {slopes[h]}: rel_err {err:.3e}")
        assert err <= BAR
    # the zero-slope head is plain causal attention
    q, k, v = (_dev_bits(a, "bf16") for a in _qkv(*case))
    plain = _values(_host_bits(sdpa_causal(q, k, v)), "bf16")
    assert rel_err(got[1], plain[1]) <= BAR
    assert rel_err(got[0], plain[0]) >= FAR


@pytest.mark.parametrize("hq,hkv,q_len,kv_len,d,dtype", CASES)
def test_sdpa_alibi_really_applies_the_bias(hq, hkv, q_len, kv_len, d, dtype):
    """All-zero slopes: far from the real-slopes oracle, inside the bar of the zero-slope oracle."""
    zero = (0.0,) * hq
    got = _run(hq, hkv, q_len, kv_len, d, dtype, zero)
    away = rel_err(got, _oracle(hq, hkv, q_len, kv_len, d, dtype, _std_slopes(hq)))
    near = rel_err(got, _oracle(hq, hkv, q_len, kv_len, d, dtype, zero))
    print(f"zero slopes ({hq},{hkv}) q {q_len} kv {kv_len}: {away:.3e} from the oracle, {near:.3e} from the zero-slope oracle")
    assert away >= FAR
    assert near <= BAR


def test_sdpa_alibi_slopes_belong_to_query_heads():
    case = (8, 2, 129, 333, 128, "bf16")
    slopes = _std_slopes(8)
    want = _oracle(*case, slopes)
    got = _run(*case, slopes)
    for h in range(8):
        err = rel_err(got[h], want[h])
        print(f"head {h}: rel_err {err:.3e}")
        assert err <= BAR
    away = rel_err(_run(*case, slopes[::-1]), want)
    print(f"reversed slopes: {away:.3e} from the oracle")
    assert away >= FAR


def test_sdpa_alibi_equals_attention_over_the_materialised_bias():
    from pygpukit_amd.ops.nn import alibi_compute_bias

    case = (4, 2, 70, 70, 128, "bf16")
    slopes = _std_slopes(4)
    bias = alibi_compute_bias(70, 4, _dev(np.array(slopes, np.float32))).to_numpy()
    q, k, v = (_values(a, "bf16") for a in _qkv(*case))
    err = rel_err(_run(*case, slopes), P.sdpa_with_bias(q, k, v, bias))
    print(f"sdpa_alibi against softmax(QK^T scale + alibi_compute_bias) V: rel_err {err:.3e}")
    assert err <= BAR


def test_sdpa_alibi_strided_is_bit_identical_to_the_contiguous_call():
    from pygpukit_amd.ops.nn import sdpa_alibi, sdpa_alibi_strided

    hq, hkv, q_len, kv_len, d = 8, 2, 129, 333, 128
    qw, kw, vw = _qkv(hq, hkv, q_len, kv_len, d, "bf16")
    slopes = _dev(P.alibi_init_slopes(hq))
    k, v = _dev_bits(kw, "bf16"), _dev_bits(vw, "bf16")
    want = _host_bits(sdpa_alibi(_dev_bits(qw, "bf16"), k, v, slopes))
    q_shd = _dev_bits(np.ascontiguousarray(qw.transpose(1, 0, 2)), "bf16")          # [S, H, D]
    out = _nan_out((q_len, hq, d), "bf16")
    sdpa_alibi_strided(q_shd, k, v, slopes, out, hq, hkv, q_len, kv_len, d, (d, hq * d), (kv_len * d, d), (d, hq * d))
    np.testing.assert_array_equal(_host_bits(out).transpose(1, 0, 2), want)


# ---- sdpa_alibi_fixed_cache --------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _cache_qkv(hq, hkv, d, dtype, q_len=1, max_seq=MAX_SEQ):
    rng = np.random.default_rng(7000 + 100 * hq + 10 * hkv + d + q_len)
    q, k, v = (_bits(rng.standard_normal(s).astype(np.float32), dtype) for s in ((hq, q_len, d), (hkv, max_seq, d), (hkv, max_seq, d)))
    for a in (q, k, v):
        a.setflags(write=False)
    return q, k, v


@functools.lru_cache(maxsize=None)
def _cache_want(hq, hkv, d, dtype, ctx, q_len=1, zero=False, max_seq=MAX_SEQ):
    q, k, v = (_values(a, dtype) for a in _cache_qkv(hq, hkv, d, dtype, q_len, max_seq))
    slopes = np.zeros(hq, np.float32) if zero else P.alibi_init_slopes(hq)
    want = P.sdpa_alibi(q, k[:, :ctx], v[:, :ctx], slopes)
    want.setflags(write=False)
    return want


def _caches(hq, hkv, d, dtype, ctx, q_len=1, max_seq=MAX_SEQ):
    """Device Q and caches whose rows from `ctx` on hold NaN: a kernel that reads one row too many returns NaN."""
    q, k, v = _cache_qkv(hq, hkv, d, dtype, q_len, max_seq)
    k, v = k.copy(), v.copy()
    k[:, ctx:] = NAN_BITS[dtype]
    v[:, ctx:] = NAN_BITS[dtype]
    return _dev_bits(q, dtype), _dev_bits(k, dtype), _dev_bits(v, dtype)


def _attend(hq, hkv, d, dtype, ctx, q_len=1, zero=False, max_seq=MAX_SEQ):
    from pygpukit_amd.ops.nn import sdpa_alibi_fixed_cache

    qd, kd, vd = _caches(hq, hkv, d, dtype, ctx, q_len, max_seq)
    out = _nan_out((hq, q_len, d), dtype)
    slopes = np.zeros(hq, np.float32) if zero else P.alibi_init_slopes(hq)
    sdpa_alibi_fixed_cache(qd, kd, vd, _dev(slopes), out, ctx)
    words = _host_bits(out)
    assert np.isfinite(_values(words, dtype)).all()
    return words


@pytest.mark.parametrize("ctx", [1, 17, 70, 256, 257, 1024])      # three empty splits .. first row of the second chunk .. full cache
def test_fixed_cache_attention_matches_the_restatement_at_every_split_boundary(ctx):
    err = rel_err(_values(_attend(4, 2, 128, "bf16", ctx), "bf16"), _cache_want(4, 2, 128, "bf16", ctx))
    print(f"sdpa_alibi_fixed_cache (4,2) D 128 context {ctx}: rel_err {err:.3e}")
    assert err <= BAR


@pytest.mark.parametrize("hq,hkv", [(2, 2), (4, 2), (8, 2), (5, 1), (40, 8)])      # Hq / Hkv = 1, 2, 4, 5, 5
def test_fixed_cache_attention_every_head_grouping(hq, hkv):
    got, want = _values(_attend(hq, hkv, 128, "bf16", 300), "bf16"), _cache_want(hq, hkv, 128, "bf16", 300)
    err = rel_err(got, want)
    print(f"sdpa_alibi_fixed_cache ({hq},{hkv}) D 128 context 300: rel_err {err:.3e}")
    assert err <= BAR
    assert max(rel_err(got[h], want[h]) for h in range(hq)) <= BAR          # every head has its own slope


def test_fixed_cache_attention_five_heads_per_workgroup():
    """Hq / Hkv = 5 takes the five-heads-per-workgroup kernel only where that grid has 256 workgroups: 40 / 8 heads need
    32 KV splits, a cache of 8192 rows (at MAX_SEQ the case above runs one head per workgroup)."""
    got = _values(_attend(40, 8, 128, "bf16", 300, max_seq=8192), "bf16")
    want = _cache_want(40, 8, 128, "bf16", 300, max_seq=8192)
    err = rel_err(got, want)
    print(f"sdpa_alibi_fixed_cache (40,8) D 128 cache 8192 context 300: rel_err {err:.3e}")
    assert err <= BAR
    assert max(rel_err(got[h], want[h]) for h in range(40)) <= BAR


def test_fixed_cache_attention_head_dim_64_float16():
    err = rel_err(_values(_attend(4, 2, 64, "f16", 300), "f16"), _cache_want(4, 2, 64, "f16", 300))
    print(f"sdpa_alibi_fixed_cache (4,2) D 64 f16 context 300: rel_err {err:.3e}")
    assert err <= BAR


def test_fixed_cache_attention_five_query_rows_run_the_prefill_kernel_over_the_cache():
    err = rel_err(_values(_attend(4, 2, 128, "bf16", 75, q_len=5), "bf16"), _cache_want(4, 2, 128, "bf16", 75, q_len=5))
    print(f"sdpa_alibi_fixed_cache (4,2) D 128 q_len 5 context 75: rel_err {err:.3e}")
    assert err <= BAR


def test_fixed_cache_attention_really_applies_the_bias():
    got = _values(_attend(4, 2, 128, "bf16", 1024, zero=True), "bf16")
    away, near = rel_err(got, _cache_want(4, 2, 128, "bf16", 1024)), rel_err(got, _cache_want(4, 2, 128, "bf16", 1024, zero=True))
    print(f"zero slopes at context 1024: {away:.3e} from the oracle, {near:.3e} from the zero-slope oracle")
    assert away >= FAR
    assert near <= BAR


def test_fixed_cache_attention_ptr_form_and_graph_replay_are_bit_identical():
    import pygpukit_amd as pk
    from pygpukit_amd.ops.nn import sdpa_alibi_fixed_cache_ptr

    slopes = _dev(P.alibi_init_slopes(4))
    host = {ctx: _attend(4, 2, 128, "bf16", ctx) for ctx in (70, 257)}
    for ctx in (70, 257):
        qd, kd, vd = _caches(4, 2, 128, "bf16", ctx)
        out = _nan_out((4, 1, 128), "bf16")
        sdpa_alibi_fixed_cache_ptr(qd, kd, vd, slopes, out, _i32(ctx), MAX_SEQ)
        np.testing.assert_array_equal(_host_bits(out), host[ctx])
    # captured once with 70 in the device buffer (a single chain of two kernels), replayed, then replayed after the buffer
    # is rewritten to 257; the caches hold rows 0 .. 256 (NaN beyond), which both contexts may read
    qd, kd, vd = _caches(4, 2, 128, "bf16", 257)
    out, cbuf = _nan_out((4, 1, 128), "bf16"), _i32(70)
    graph = pk.CudaGraph()
    graph.begin_capture()
    sdpa_alibi_fixed_cache_ptr(qd, kd, vd, slopes, out, cbuf, MAX_SEQ)
    graph.end_capture()
    graph.replay()
    graph.synchronize()
    np.testing.assert_array_equal(_host_bits(out), host[70])
    cbuf.copy_from_numpy(np.array([257], np.int32))
    graph.replay()
    graph.synchronize()
    np.testing.assert_array_equal(_host_bits(out), host[257])


# ---- refused cases -----------------------------------------------------------------------------------------------------

def test_refused_cases():
    from pygpukit_amd import _hip
    from pygpukit_amd.core import from_numpy
    from pygpukit_amd.ops.nn import (alibi_add_bias, alibi_compute_bias, pope_inplace, sdpa_alibi, sdpa_alibi_fixed_cache,
                                     sdpa_alibi_fixed_cache_ptr, sdpa_alibi_strided)

    bf = lambda *s: from_numpy(np.zeros(s, np.uint16))       # noqa: E731
    f32 = lambda *s: from_numpy(np.zeros(s, np.float32))     # noqa: E731
    sl4 = f32(4)
    with pytest.raises(ValueError, match="float16/bfloat16"):
        sdpa_alibi(f32(4, 8, 128), f32(2, 8, 128), f32(2, 8, 128), sl4)
    with pytest.raises(ValueError, match="head_dim"):
        sdpa_alibi(bf(4, 8, 96), bf(2, 8, 96), bf(2, 8, 96), sl4)
    with pytest.raises(ValueError, match="n_heads"):
        sdpa_alibi(bf(3, 8, 128), bf(2, 8, 128), bf(2, 8, 128), f32(3))
    with pytest.raises(ValueError, match="kv_len >= q_len"):
        sdpa_alibi(bf(4, 8, 128), bf(2, 7, 128), bf(2, 7, 128), sl4)
    with pytest.raises(ValueError, match="slopes must be float32"):
        sdpa_alibi(bf(4, 8, 128), bf(2, 8, 128), bf(2, 8, 128), bf(4))
    with pytest.raises(ValueError, match="slopes must have 4"):
        sdpa_alibi(bf(4, 8, 128), bf(2, 8, 128), bf(2, 8, 128), f32(2))          # one per kv head is not enough
    with pytest.raises(ValueError, match="multiples of 8"):
        sdpa_alibi_strided(bf(8, 4, 128), bf(2, 8, 128), bf(2, 8, 128), sl4, bf(8, 4, 128), 4, 2, 8, 8, 128, (128, 516), (1024, 128), (128, 512))
    with pytest.raises(ValueError, match="slopes must have 4"):
        sdpa_alibi_fixed_cache(bf(4, 1, 128), bf(2, 64, 128), bf(2, 64, 128), f32(2), bf(4, 1, 128), 3)
    with pytest.raises(ValueError, match="outside cache"):
        sdpa_alibi_fixed_cache(bf(4, 1, 128), bf(2, 64, 128), bf(2, 64, 128), sl4, bf(4, 1, 128), 65)
    with pytest.raises(ValueError, match="kv_len >= q_len"):
        sdpa_alibi_fixed_cache(bf(4, 5, 128), bf(2, 64, 128), bf(2, 64, 128), sl4, bf(4, 5, 128), 4)          # context < q_len
    with pytest.raises(ValueError, match="q_len must be 1"):
        sdpa_alibi_fixed_cache_ptr(bf(4, 5, 128), bf(2, 64, 128), bf(2, 64, 128), sl4, bf(4, 5, 128), _i32(9), 64)
    with pytest.raises(ValueError, match="int32"):
        sdpa_alibi_fixed_cache_ptr(bf(4, 1, 128), bf(2, 64, 128), bf(2, 64, 128), sl4, bf(4, 1, 128), f32(1), 64)
    with pytest.raises(ValueError, match="outside the encoding table"):
        pope_inplace(f32(5, 3, 8), f32(5, 1, 8), f32(16, 8), start_pos=12)
    with pytest.raises(ValueError, match="outside the encoding table"):
        pope_inplace(f32(5, 3, 8), f32(5, 1, 8), f32(16, 8), start_pos=-1)
    with pytest.raises(ValueError, match="encoding must be float32"):
        pope_inplace(bf(5, 3, 8), bf(5, 1, 8), bf(16, 8))
    with pytest.raises(ValueError, match="scores must be float32"):
        alibi_add_bias(bf(1, 4, 2, 2), sl4)
    with pytest.raises(ValueError, match="slopes must be float32"):
        alibi_add_bias(f32(1, 4, 2, 2), bf(4))
    with pytest.raises(ValueError, match="slopes must have 4"):
        alibi_add_bias(f32(1, 4, 2, 2), f32(3))
    with pytest.raises(ValueError, match="slopes must have 4"):
        alibi_compute_bias(5, 4, f32(8))

    # the native entries refuse the same on their own, with a message
    q, kc, o, ws, enc = bf(4, 8, 128), bf(2, 64, 128), bf(4, 8, 128), f32(4 * 130), f32(16, 8)
    BF16, F32 = q.dtype.code, ws.dtype.code

    def prefill(hq=4, hkv=2, q_len=8, kv_len=8, d=128, dt=BF16, qs=128):
        _hip.call("pgk_sdpa_alibi", q._p, kc._p, kc._p, sl4._p, o._p, hq, hkv, q_len, kv_len, d, 0.0, q_len * d, qs, 64 * d, d, q_len * d, d, dt, None)

    def cached(hq=4, hkv=2, q_len=1, d=128, ctx=3, dt=BF16, buf=None):
        _hip.call("pgk_sdpa_alibi_fixed_cache", q._p, kc._p, kc._p, sl4._p, o._p, hq, hkv, q_len, 64, d, 0.0, ctx, buf, ws._p, dt, None)

    for fn, name in ((prefill, "pgk_sdpa_alibi"), (cached, "pgk_sdpa_alibi_fixed_cache")):
        with pytest.raises(RuntimeError, match=name + ": float16 / bfloat16 only"):
            fn(dt=F32)
        with pytest.raises(RuntimeError, match=name + ": head_dim must be 64 or 128"):
            fn(d=96)
        with pytest.raises(RuntimeError, match=name + ": n_heads mismatch"):
            fn(hq=3)
    with pytest.raises(RuntimeError, match="kv_len >= q_len"):
        prefill(kv_len=7)
    with pytest.raises(RuntimeError, match="multiples of 8"):
        prefill(qs=132)
    with pytest.raises(RuntimeError, match="invalid context_len"):
        cached(ctx=65)
    with pytest.raises(RuntimeError, match="invalid context_len"):
        cached(q_len=5, ctx=4)
    with pytest.raises(RuntimeError, match="requires q_len == 1"):
        cached(q_len=5, ctx=9, buf=_i32(9)._p)
    with pytest.raises(RuntimeError, match="outside the encoding table"):
        _hip.call("pgk_pope_inplace", ws._p, ws._p, enc._p, 5, 3, 1, 8, 12, 16, F32, None)
    with pytest.raises(RuntimeError, match="outside the encoding table"):
        _hip.call("pgk_pope_inplace", ws._p, ws._p, enc._p, 5, 3, 1, 8, -1, 16, F32, None)
    with pytest.raises(RuntimeError, match="must be float32"):
        _hip.call("pgk_alibi_add_bias", ws._p, sl4._p, 1, 4, 2, 2, 0, BF16, F32, 4, None)
    with pytest.raises(RuntimeError, match="3 slopes for 4 heads"):
        _hip.call("pgk_alibi_add_bias", ws._p, sl4._p, 1, 4, 2, 2, 0, F32, F32, 3, None)
    prefill()          # and accept the valid calls
    cached()
    cached(q_len=5, ctx=9)
