"""ln_linear, ln_linear_qkv_cache_ptr and embed_token_position_ptr on the GPU against the float64 oracle of
tests/whisper_decoder_ref.py, elementwise, on the values the device holds (rounded to the dtype first).

The bar is derived, not measured (R.ln_bar):
    accumulation  |err| <= (n + n_ln) 2^-24 (sum |x^ w| + |b| + |r|), n = K + 2 (doubled in float32, whose products round),
                  n_ln = 0 without the norm and 2K + 8 with it: two K-term fp32 sums and the normalisation's roundings move each
                  x^ by at most that many ulps.  n_ln = 2K + 8 was kept as derived: the float32 NumPy restatement (not the code under
                  test) stays inside the bar on every case, worst |err| / bar 0.041 in float32, 0.979 in bfloat16 and 0.948 in
                  float16, where the output rounding alone may reach 1 (tests/test_whisper_decoder_cpu.py)
    GELU          the pre-activation bar x 1.13 (the largest |gelu'|) + 2^-21 |ref| for the device tanhf
    output        + 2^-8 |ref| in bfloat16, 2^-11 |ref| in float16, nothing in float32.
LN cases draw x ~ N(0.3, 1), so that x - mean does not cancel.  The shapes reach every path ln_linear_plan names (asserted per case),
the chunk boundaries of the peeled first trip, row tails at every grouping and more than one workgroup; the dispatcher has no K
specialisation to list (LN_LINEAR_K_SPECIALIZATIONS is empty)."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from tests import whisper_decoder_ref as R

pytestmark = pytest.mark.gpu

DTYPES = ("f32", "bf16", "f16")
# the path each (shape, norm?) takes per dtype class; everything else is "fp32_image"
EXPECT = {((3, 204, 37), False): "generic", ((3, 204, 37), True): "generic",
          ((8, 5120, 16), False): "generic", ((8, 5120, 16), True): "generic",
          ((4, 5120, 24), True): "generic"}


def _pk(dtype):
    from pygpukit_amd.core.dtypes import bfloat16, float16, float32

    return {"f32": float32, "bf16": bfloat16, "f16": float16}[dtype]


def _dev(x, dtype):
    from pygpukit_amd.core import from_numpy

    if x is None:
        return None
    w = R.to_words(x, dtype)
    return from_numpy(np.ascontiguousarray(w.view(np.float16) if dtype == "f16" else w))


def _words(a, dtype):
    h = a.to_numpy()
    return h if dtype == "f32" or h.dtype == np.uint16 else h.view(np.uint16)


def _host(a, dtype):
    return R.from_words(_words(a, dtype), dtype).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _case(shape, variant, dtype):
    """Operands as the device holds them, the float64 result and the bar - computed once per case and left unchanged."""
    c = R.make_ln_case(shape, variant, dtype)
    ref, bar = R.ln_linear(c), R.ln_bar(c, dtype)
    for a in (ref, bar):
        a.setflags(write=False)
    return c, ref, bar


def _expected_plan(shape, norm, dtype):
    if (shape, norm) in EXPECT:
        return EXPECT[(shape, norm)]
    if shape == (4, 5120, 24):                       # no norm: fp32 image 80 KB
        return "generic" if dtype == "f32" else "dtype_image"
    return "fp32_image"


def _run(c, dtype, variant, misalign=False):
    from pygpukit_amd.core.array import GPUArray
    from pygpukit_amd.ops.nn.linear import ln_linear

    x = _dev(c["x"], dtype)
    if misalign:                                     # the same rows one element into a larger buffer: off 16-byte alignment
        m, k = c["x"].shape
        big = _dev(np.concatenate([np.zeros(1, np.float32), c["x"].ravel()]), dtype)
        x = big._view(1, (m, k))
    kw = dict(gamma=_dev(c["gamma"], dtype), beta=_dev(c["beta"], dtype), activation=c["activation"])
    res = _dev(c["residual"], dtype)
    if variant == "residual_alias_out":
        return ln_linear(x, _dev(c["w"], dtype), _dev(c["bias"], dtype), residual=res, out=res, **kw)
    return ln_linear(x, _dev(c["w"], dtype), _dev(c["bias"], dtype), residual=res, **kw)


def _assert_within(got, ref, bar, what):
    err = np.abs(got - ref)
    worst = float(np.max(err / np.maximum(bar, 1e-300)))
    print(f"{what}: max |err| {err.max():.3e}, max err/bar {worst:.3f}")
    assert np.all(np.isfinite(got)) and worst <= 1.0, what


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", R.LN_SHAPES, ids=str)
def test_every_variant_within_the_derived_bar(shape, dtype, monkeypatch):
    from pygpukit_amd.ops.nn.linear import ln_linear_plan

    monkeypatch.delenv("PGK_LN_LINEAR_GENERIC", raising=False)
    for variant in R.LN_VARIANTS:
        c, ref, bar = _case(shape, variant, dtype)
        norm = c["gamma"] is not None
        assert ln_linear_plan(*shape, _pk(dtype), norm=norm) == _expected_plan(shape, norm, dtype), (shape, variant)
        out = _run(c, dtype, variant)
        assert out.shape == (shape[0], shape[2])
        _assert_within(_host(out, dtype), ref, bar, f"{shape} {variant} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(1, 128, 203), (8, 128, 384), (1, 1280, 70), (2, 5120, 40)], ids=str)
def test_generic_path_forced_agrees_within_the_same_bar(shape, dtype, monkeypatch):
    from pygpukit_amd.ops.nn.linear import ln_linear_plan

    monkeypatch.setenv("PGK_LN_LINEAR_GENERIC", "1")
    assert ln_linear_plan(*shape, _pk(dtype)) == "generic"
    for variant in ("bias", "ln_bias_gelu", "ln_bias_residual", "residual_alias_out"):
        c, ref, bar = _case(shape, variant, dtype)
        _assert_within(_host(_run(c, dtype, variant), dtype), ref, bar, f"generic {shape} {variant} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_misaligned_activations_take_the_generic_kernel(dtype, monkeypatch):
    monkeypatch.delenv("PGK_LN_LINEAR_GENERIC", raising=False)
    for variant in ("plain", "ln_bias_gelu"):
        c, ref, bar = _case((3, 200, 37), variant, dtype)
        _assert_within(_host(_run(c, dtype, variant, misalign=True), dtype), ref, bar, f"misaligned {variant} {dtype}")


# ---- exact checks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 128, 203), (8, 128, 384), (1, 1280, 70), (3, 204, 37)], ids=str)
def test_float32_epilogue_equals_the_ops_bit_for_bit(shape):
    """Fused GELU = the gelu op on the unfused result, fused residual = the add op on it: one fp32 function, one fp32 add."""
    from pygpukit_amd.ops.elementwise import add
    from pygpukit_amd.ops.nn.activation import gelu
    from pygpukit_amd.ops.nn.linear import ln_linear

    c, _, _ = _case(shape, "ln_bias_gelu", "f32")
    x, w, b, g, be = (_dev(c[k], "f32") for k in ("x", "w", "bias", "gamma", "beta"))
    plain = ln_linear(x, w, b, gamma=g, beta=be)
    fused = ln_linear(x, w, b, gamma=g, beta=be, activation="gelu")
    assert np.array_equal(_words(fused, "f32").view(np.uint32), _words(gelu(plain), "f32").view(np.uint32))
    r = _dev(np.random.default_rng(5).standard_normal((shape[0], shape[2])).astype(np.float32), "f32")
    with_r = ln_linear(x, w, b, gamma=g, beta=be, residual=r)
    assert np.array_equal(_words(with_r, "f32").view(np.uint32), _words(add(plain, r), "f32").view(np.uint32))
    both = ln_linear(x, w, b, gamma=g, beta=be, activation="gelu", residual=r)
    assert np.array_equal(_words(both, "f32").view(np.uint32), _words(add(gelu(plain), r), "f32").view(np.uint32))


QKV = dict(k=128, heads=2, head_dim=64, max_seq=24)


@functools.lru_cache(maxsize=None)
def _qkv_case(dtype, k):
    rng = np.random.default_rng(77 + k)
    d = QKV["heads"] * QKV["head_dim"]
    c = dict(x=0.3 + rng.standard_normal((1, k)), w=rng.standard_normal((3 * d, k)) / np.sqrt(k), bias=0.5 * rng.standard_normal(3 * d),
             gamma=1.0 + 0.1 * rng.standard_normal(k), beta=0.1 * rng.standard_normal(k))
    return {key: R.round_to(v.astype(np.float32), dtype) for key, v in c.items()}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [128, 204], ids=["fast", "generic"])
def test_qkv_cache_equals_ln_linear_plus_two_cache_writes_bit_for_bit(dtype, k):
    from pygpukit_amd.core import from_numpy
    from pygpukit_amd.core.array import GPUArray
    from pygpukit_amd.ops.embedding import kv_cache_update_gqa
    from pygpukit_amd.ops.nn.linear import ln_linear, ln_linear_qkv_cache_ptr

    H, hd, T = QKV["heads"], QKV["head_dim"], QKV["max_seq"]
    d = H * hd
    c = _qkv_case(dtype, k)
    x, w, b, g, be = (_dev(c[key], dtype) for key in ("x", "w", "bias", "gamma", "beta"))
    sentinel = R.round_to(np.full((H, T, hd), -7.25, np.float32), dtype)
    want_qkv = ln_linear(x, w, b, gamma=g, beta=be)
    wq = _words(want_qkv, dtype).ravel()
    for pos in (0, 5, T - 1):
        want_k, want_v = _dev(sentinel, dtype), _dev(sentinel, dtype)
        kv_cache_update_gqa(want_qkv._view(d, (1, H, hd)), want_k, H, pos)
        kv_cache_update_gqa(want_qkv._view(2 * d, (1, H, hd)), want_v, H, pos)
        for through_buffer in (True, False):
            q, kc, vc = GPUArray((1, d), _pk(dtype)), _dev(sentinel, dtype), _dev(sentinel, dtype)
            if through_buffer:
                ln_linear_qkv_cache_ptr(x, w, b, q, kc, vc, from_numpy(np.array([pos], np.int32)), gamma=g, beta=be)
            else:
                ln_linear_qkv_cache_ptr(x, w, b, q, kc, vc, gamma=g, beta=be, position=pos)
            assert np.array_equal(_words(q, dtype).ravel(), wq[:d]), (pos, through_buffer)
            for got, want, part in ((kc, want_k, 1), (vc, want_v, 2)):
                gw = _words(got, dtype)
                assert np.array_equal(gw, _words(want, dtype)), (pos, through_buffer, part)
                assert np.array_equal(gw[:, pos].ravel(), wq[part * d:(part + 1) * d])                 # the row itself ...
                others = np.delete(gw, pos, axis=1)
                assert np.array_equal(others, np.delete(R.to_words(sentinel, dtype), pos, axis=1))     # ... and nothing else


@pytest.mark.parametrize("dtype", DTYPES)
def test_qkv_cache_device_position_is_clamped_to_the_cache(dtype):
    """A position outside the cache read from the device lands on the nearest row: never outside the allocation."""
    from pygpukit_amd.core import from_numpy
    from pygpukit_amd.core.array import GPUArray
    from pygpukit_amd.ops.nn.linear import ln_linear_qkv_cache_ptr

    H, hd, T = QKV["heads"], QKV["head_dim"], QKV["max_seq"]
    c = _qkv_case(dtype, 128)
    x, w, b = (_dev(c[key], dtype) for key in ("x", "w", "bias"))
    sentinel = R.round_to(np.full((H, T, hd), -7.25, np.float32), dtype)
    for pos, row in ((T + 5, T - 1), (-3, 0)):
        q, kc, vc = GPUArray((1, H * hd), _pk(dtype)), _dev(sentinel, dtype), _dev(sentinel, dtype)
        ln_linear_qkv_cache_ptr(x, w, b, q, kc, vc, from_numpy(np.array([pos], np.int32)))
        gw = _words(kc, dtype)
        assert not np.array_equal(gw[:, row], R.to_words(sentinel, dtype)[:, row])
        assert np.array_equal(np.delete(gw, row, axis=1), np.delete(R.to_words(sentinel, dtype), row, axis=1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_embed_token_position_is_one_add_and_one_rounding(dtype):
    from pygpukit_amd.core import from_numpy
    from pygpukit_amd.core.array import GPUArray
    from pygpukit_amd.ops.nn.linear import embed_token_position_ptr

    rng = np.random.default_rng(12)
    V, P, d = 203, 24, 136                                   # d: no multiple of the block
    tok = R.round_to(rng.standard_normal((V, d)).astype(np.float32), dtype)
    pos = R.round_to(rng.standard_normal((P, d)).astype(np.float32), dtype)
    dt, dp = _dev(tok, dtype), _dev(pos, dtype)
    for (t, p), (ct, cp) in (((0, 0), (0, 0)), ((V - 1, P - 1), (V - 1, P - 1)), ((7, 3), (7, 3)), ((V + 9, P), (V - 1, P - 1)), ((-1, -5), (0, 0))):
        out = GPUArray((1, d), _pk(dtype))
        embed_token_position_ptr(dt, dp, out, from_numpy(np.array([t, p, p + 1], np.int32)))
        want = R.to_words(tok[ct].astype(np.float32) + pos[cp].astype(np.float32), dtype)          # fp32 add, one rounding
        assert np.array_equal(_words(out, dtype).ravel(), want.ravel()), (t, p)
