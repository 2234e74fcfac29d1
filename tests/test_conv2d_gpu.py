"""conv2d on the GPU against the float64 direct sum of tests/vae_ref.py, element by element, on every tail of both kernels.

The bar is derived, not measured (tests/test_conv1d_gpu.py).  The oracle runs on exactly the values the device holds.  Products
of 16-bit inputs are exact in fp32, so any fp32 summation order of n = C_in KH KW + 1 terms obeys
    |err| <= n 2^-24 (sum |x w| + |b|)                              per output element,
plus the rounding of the result, 2^-8 |ref| in bfloat16 and 2^-11 |ref| in float16, and nothing in float32, where the
accumulation term is doubled for the rounded fp32 products.  tests/test_vae_cpu.py shows that a dropped tap, a padding off by one
and a missing upsample shift move a result by tens of percent.  Layout, upsample, packed-weight and float32 `add=` variants
must reproduce the plain call bit for bit: they change an index computation or add one exactly specified term.

The MFMA kernel has two patch heights.  Its launcher picks 16 rows only when the grid covers the chip twice, which no quick test
shape does, so test_conv2d_16_row_kernel forces them with PGK_CONV2D_ROWS=16 on the ragged, the 1x1 and the tiny-channel case -
plain, channels-last, upsample=2 and add= - against the same derived bars, and requires bit-identity with the 8-row result: both
heights accumulate an output element over (chunk, tap, k-step) in the same order."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from tests import vae_ref as R

pytestmark = pytest.mark.gpu

DTYPES = ("float32", "bfloat16", "float16")
OUT_EPS = {"float32": 0.0, "bfloat16": 2.0 ** -8, "float16": 2.0 ** -11}
IDS = [str(c) for c in R.CONV_CASES]


def _dev(a, dtype):
    """Upload values already rounded to `dtype` (the device cast is then exact)."""
    from pygpukit_amd.core import from_numpy
    from pygpukit_amd.core.dtypes import as_dtype

    return None if a is None else from_numpy(np.ascontiguousarray(a, dtype=np.float32)).astype(as_dtype(dtype))


def _host(a):
    from pygpukit_amd.core.dtypes import float32

    return a.astype(float32).to_numpy()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@functools.lru_cache(maxsize=None)
def _case(i, dtype):
    """Inputs as the device holds them, the float64 result and the accumulation term of the bar - computed once per case."""
    case = R.CONV_CASES[i]
    x, w, b = (R.round_to(a.astype(np.float64), dtype) for a in R.conv_inputs(i))
    s, p, d = case[6:9]
    ref = R.conv2d(x, w, b, s, p, d)
    n = case[1] * case[5] * case[5] + 1
    acc = (2.0 if dtype == "float32" else 1.0) * n * 2.0 ** -24 * R.conv2d(x, w, b, s, p, d, absolute=True)
    for a in (x, w, b, ref, acc):
        a.setflags(write=False)
    return x, w, b, ref, acc


def _run(i, dtype, x=None, **kw):
    from pygpukit_amd.ops.conv import conv2d

    cx, w, b, _, _ = _case(i, dtype)
    s, p, d = R.CONV_CASES[i][6:9]
    return conv2d(_dev(cx if x is None else x, dtype), _dev(w, dtype), _dev(b, dtype), s, p, d, **kw)


def _assert_within(got, ref, bar, what):
    err = np.abs(got - ref)
    worst = float(np.max(err / np.maximum(bar, 1e-300)))
    print(f"{what}: max |err| {err.max():.3e}, max err/bar {worst:.3f}")
    assert got.shape == ref.shape and np.all(err <= bar), f"{what}: {int((err > bar).sum())} of {err.size} elements beyond the bar, worst {worst:.2f} x"


def _plan(i, dtype):
    from pygpukit_amd.ops.conv import conv2d_plan

    c = R.CONV_CASES[i]
    return conv2d_plan(c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("i", range(len(R.CONV_CASES)), ids=IDS)
def test_conv2d_matches_the_direct_sum(i, dtype):
    assert _plan(i, dtype) == ("fma" if dtype == "float32" else R.CONV_PLANS_16[i])
    _, _, _, ref, acc = _case(i, dtype)
    _assert_within(_host(_run(i, dtype)).astype(np.float64), ref, acc + OUT_EPS[dtype] * np.abs(ref), f"conv2d {R.CONV_CASES[i]} {dtype}")


@pytest.mark.parametrize("dtype", ("bfloat16", "float16"))
@pytest.mark.parametrize("i", (1, 4), ids=[IDS[1], IDS[4]])
def test_conv2d_16bit_on_the_forced_fma_kernel(i, dtype, monkeypatch):
    monkeypatch.setenv("PGK_CONV_MFMA", "0")
    assert _plan(i, dtype) == "fma"
    _, _, _, ref, acc = _case(i, dtype)
    _assert_within(_host(_run(i, dtype)).astype(np.float64), ref, acc + OUT_EPS[dtype] * np.abs(ref), f"conv2d fma {R.CONV_CASES[i]} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("i", (1, 3, 4), ids=[IDS[1], IDS[3], IDS[4]])
def test_conv2d_layouts_are_bit_identical(i, dtype):
    """(1): C_in = 40, C_out = 70 - the vector paths of the channels-last fill (C_in % 8 == 0) and never of the store (70 % 4 != 0);
    (3): C_in = 33 - the scalar channels-last fill, C_out = 64 - the 4-channel store; (4): 8 -> 8, stride 2, both vector paths."""
    x = _case(i, dtype)[0]
    plain = _host(_run(i, dtype))
    x_cl = np.ascontiguousarray(x.transpose(0, 2, 3, 1))
    assert _same_bits(_host(_run(i, dtype, x_cl, channels_last=True)), plain)
    assert _same_bits(_host(_run(i, dtype, channels_last_out=True)).transpose(0, 3, 1, 2), plain)
    assert _same_bits(_host(_run(i, dtype, x_cl, channels_last=True, channels_last_out=True)).transpose(0, 3, 1, 2), plain)


@pytest.mark.parametrize("channels_last", (False, True))
@pytest.mark.parametrize("dtype", DTYPES)
def test_conv2d_upsample_is_the_conv_of_the_upsampled_input(dtype, channels_last):
    """Odd H and W (11 x 19 -> 22 x 38): two patches each way, the (y >> 1, x >> 1) index and the border are all exercised."""
    x = _case(1, dtype)[0]
    up = R.upsample2(x)
    tr = (lambda a: np.ascontiguousarray(a.transpose(0, 2, 3, 1))) if channels_last else (lambda a: a)
    got = _host(_run(1, dtype, tr(x), upsample=2, channels_last=channels_last))
    want = _host(_run(1, dtype, tr(up), channels_last=channels_last))
    assert got.shape == (2, 70, 22, 38) and _same_bits(got, want)


@pytest.mark.parametrize("channels_last_out", (False, True))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("i", (1, 4), ids=[IDS[1], IDS[4]])
def test_conv2d_add(i, dtype, channels_last_out):
    from pygpukit_amd.ops.elementwise import add

    _, _, _, ref, acc = _case(i, dtype)
    res = R.round_to(np.random.default_rng(50 + i).standard_normal(ref.shape), dtype)
    tr = (lambda a: np.ascontiguousarray(a.transpose(0, 2, 3, 1))) if channels_last_out else (lambda a: a)
    back = (lambda a: a.transpose(0, 3, 1, 2)) if channels_last_out else (lambda a: a)
    r_dev = _dev(tr(res), dtype)
    got = back(_host(_run(i, dtype, add=r_dev, channels_last_out=channels_last_out)))
    if dtype == "float32":
        assert _same_bits(got, back(_host(add(_run(i, dtype, channels_last_out=channels_last_out), r_dev))))
    total = ref + res
    bar = acc + (2.0 ** -24 + OUT_EPS[dtype]) * np.abs(total) + (2.0 ** -24 * (np.abs(ref) + np.abs(res)) if dtype == "float32" else 0)
    _assert_within(got.astype(np.float64), total, bar, f"conv2d add {R.CONV_CASES[i]} {dtype}")


@pytest.mark.parametrize("dtype", ("bfloat16", "float16"))
@pytest.mark.parametrize("i", (1, 3, 4), ids=[IDS[1], IDS[3], IDS[4]])
def test_conv2d_packed_weight(i, dtype):
    from pygpukit_amd.ops.conv import conv2d_pack_weight

    w = _case(i, dtype)[1]
    packed = conv2d_pack_weight(_dev(w, dtype))
    co, ci, kh, kw = w.shape
    want = np.zeros((kh * kw, -(-co // 64) * 64, -(-ci // 32) * 32), np.float32)
    want[:, :co, :ci] = w.reshape(co, ci, kh * kw).transpose(2, 0, 1)
    assert _same_bits(_host(packed), want)
    assert _same_bits(_host(_run(i, dtype, packed_weight=packed)), _host(_run(i, dtype)))


@pytest.mark.parametrize("dtype", ("float32", "bfloat16"))
def test_conv2d_out_is_honoured(dtype):
    from pygpukit_amd.core.array import GPUArray
    from pygpukit_amd.core.dtypes import as_dtype

    plain = _host(_run(4, dtype))
    out = GPUArray(plain.shape, as_dtype(dtype))
    assert _run(4, dtype, out=out) is out and _same_bits(_host(out), plain)
    with pytest.raises(ValueError, match="out shape"):
        _run(4, dtype, out=GPUArray((1, 8, 9, 17), as_dtype(dtype)))


@pytest.mark.parametrize("dtype", ("bfloat16", "float16"))
@pytest.mark.parametrize("i", (1, 2, 3), ids=[IDS[1], IDS[2], IDS[3]])
def test_conv2d_16_row_kernel(i, dtype, monkeypatch):
    """(1): 11 x 19 outputs - a ragged 16-row patch, two patches across, batch 2, two channel chunks, two channel blocks; with
    upsample=2 22 x 38 - two patches down, the second ragged.  (2): 3 output channels.  (3): 1 x 1, 8 rows of a 16-row patch."""
    case = R.CONV_CASES[i]
    x, w, b, ref, acc = _case(i, dtype)
    s, p, d = case[6:9]
    n = case[1] * case[5] * case[5] + 1
    res = R.round_to(np.random.default_rng(90 + i).standard_normal(ref.shape), dtype)
    x_cl = np.ascontiguousarray(x.transpose(0, 2, 3, 1))
    res_cl = _dev(np.ascontiguousarray(res.transpose(0, 2, 3, 1)), dtype)

    def variants():
        return {"plain": _host(_run(i, dtype)),
                "channels-last": _host(_run(i, dtype, x_cl, channels_last=True, channels_last_out=True)).transpose(0, 3, 1, 2),
                "add": _host(_run(i, dtype, add=_dev(res, dtype))),
                "add channels-last": _host(_run(i, dtype, x_cl, channels_last=True, channels_last_out=True, add=res_cl)).transpose(0, 3, 1, 2),
                "upsample": _host(_run(i, dtype, upsample=2)),
                "upsample channels-last": _host(_run(i, dtype, x_cl, upsample=2, channels_last=True, channels_last_out=True)).transpose(0, 3, 1, 2)}

    monkeypatch.setenv("PGK_CONV2D_ROWS", "8")
    rows8 = variants()
    monkeypatch.setenv("PGK_CONV2D_ROWS", "16")
    rows16 = variants()
    up_ref = R.conv2d(x, w, b, s, p, d, upsample=2)
    up_acc = n * 2.0 ** -24 * R.conv2d(x, w, b, s, p, d, upsample=2, absolute=True)
    total = ref + res
    bars = {"plain": (ref, acc + OUT_EPS[dtype] * np.abs(ref)),
            "add": (total, acc + (2.0 ** -24 + OUT_EPS[dtype]) * np.abs(total)),
            "upsample": (up_ref, up_acc + OUT_EPS[dtype] * np.abs(up_ref))}
    bars["channels-last"], bars["add channels-last"], bars["upsample channels-last"] = bars["plain"], bars["add"], bars["upsample"]
    for name, got in rows16.items():
        want, bar = bars[name]
        _assert_within(got.astype(np.float64), want, bar, f"conv2d 16 rows {name} {case} {dtype}")
        assert _same_bits(got, rows8[name]), f"{name}: the 16-row and the 8-row kernel differ"
