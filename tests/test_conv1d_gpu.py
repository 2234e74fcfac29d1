"""conv1d on the GPU against the float64 direct sum of tests/whisper_ref.py, elementwise, on every tail of both kernels.

The bar is derived, not measured.  The oracle runs on exactly the values the device gets (rounded to the dtype first).
Products of 16-bit inputs are exact in fp32, so any fp32 summation order of n = C_in K + 1 terms obeys
    |err| <= n 2^-24 (sum |x w| + |b|)                              per output element,
plus the rounding of the result, 2^-8 |ref| in bfloat16 and 2^-11 |ref| in float16 (the terms tests/test_lstm_gpu.py uses) and
nothing in float32, where the accumulation term is doubled for the rounded fp32 products.  tests/test_whisper_cpu.py shows that a
dropped tap, a padding off by one and an ignored stride move the result 25 times further than the widest of these bars.
conv1d_plan says which kernel a call takes: the 16-bit cases must take the MFMA kernel and float32 the FMA kernel, and two
16-bit cases run again with the FMA kernel forced."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from tests import whisper_ref as R

pytestmark = pytest.mark.gpu

DTYPES = ("f32", "bf16", "f16")
OUT_EPS = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}
NO_BIAS = (1, 8, 8, 9, 1, 1, 0)                      # this case runs without a bias


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
def _case(case, dtype):
    """Inputs as the device holds them, the float64 result and the accumulation term of the bar - computed once per case."""
    x, w, b = R.make_conv_case(case, bias=case != NO_BIAS)
    x, w, b = R.round_to(x, dtype), R.round_to(w, dtype), None if b is None else R.round_to(b, dtype)
    ref = R.conv1d(x, w, b, case[5], case[6])
    n = case[1] * case[4] + 1
    acc = (2.0 if dtype == "f32" else 1.0) * n * 2.0 ** -24 * R.conv1d(x, w, b, case[5], case[6], absolute=True)
    for a in (x, w, ref, acc):
        a.setflags(write=False)
    return x, w, b, ref, acc


def _run(case, dtype, **kw):
    from pygpukit_amd.ops.conv import conv1d

    x, w, b, _, _ = _case(case, dtype)
    return conv1d(_dev(x, dtype), _dev(w, dtype), _dev(b, dtype), case[5], case[6], **kw)


def _assert_within(got, ref, bar, what):
    err = np.abs(got - ref)
    worst = float(np.max(err / np.maximum(bar, 1e-300)))
    print(f"{what}: max |err| {err.max():.3e}, max err/bar {worst:.3f}")
    assert got.shape == ref.shape and np.all(err <= bar), f"{what}: {int((err > bar).sum())} of {err.size} elements beyond the bar, worst {worst:.2f} x"


def _plan(case, dtype):
    from pygpukit_amd.ops.conv import conv1d_plan

    return conv1d_plan(case[1], case[2], case[3], case[4], case[5], case[6], _pk(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.CONV_CASES, ids=str)
def test_conv1d_matches_the_direct_sum(case, dtype):
    assert _plan(case, dtype) == ("fma" if dtype == "f32" else "mfma")
    _, _, _, ref, acc = _case(case, dtype)
    _assert_within(_host(_run(case, dtype), dtype), ref, acc + OUT_EPS[dtype] * np.abs(ref), f"conv1d {case} {dtype}")


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("case", [R.CONV_CASES[1], R.CONV_CASES[4]], ids=str)
def test_16bit_calls_on_the_forced_fma_kernel(case, dtype, monkeypatch):
    monkeypatch.setenv("PGK_CONV_MFMA", "0")
    assert _plan(case, dtype) == "fma"
    _, _, _, ref, acc = _case(case, dtype)
    _assert_within(_host(_run(case, dtype), dtype), ref, acc + OUT_EPS[dtype] * np.abs(ref), f"conv1d fma {case} {dtype}")


def test_many_taps_and_a_long_stride_take_the_fma_kernel_in_16_bit():
    """K = 13 (two tap stages of the FMA kernel) and stride 10 are beyond the MFMA kernel's LDS: conv1d_plan says so and the
    result obeys the same bar."""
    for case in ((1, 9, 6, 40, 13, 1, 6), (1, 10, 70, 700, 3, 10, 1)):
        assert _plan(case, "bf16") == "fma"
        _, _, _, ref, acc = _case(case, "bf16")
        _assert_within(_host(_run(case, "bf16"), "bf16"), ref, acc + OUT_EPS["bf16"] * np.abs(ref), f"conv1d {case} bf16")


# ---- epilogue ---------------------------------------------------------------------------------------------------------
EPI_CASES = (R.CONV_CASES[1], R.CONV_CASES[2], R.CONV_CASES[5])


@pytest.mark.parametrize("case", EPI_CASES, ids=str)
def test_float32_fused_gelu_is_the_gelu_op_bit_for_bit(case):
    from pygpukit_amd.ops.nn import gelu

    fused = _run(case, "f32", activation="gelu").to_numpy()
    np.testing.assert_array_equal(fused.view(np.uint32), gelu(_run(case, "f32")).to_numpy().view(np.uint32))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", EPI_CASES, ids=str)
def test_channels_last_is_the_transposed_result_bit_for_bit(case, dtype):
    plain = _words(_run(case, dtype, activation="gelu"), dtype)
    last = _words(_run(case, dtype, activation="gelu", channels_last_out=True), dtype)
    assert last.shape == (plain.shape[0], plain.shape[2], plain.shape[1])
    np.testing.assert_array_equal(last, plain.transpose(0, 2, 1))


def _add_operand(case, dtype):
    l_out = R.conv_out_length(case[3], case[4], case[5], case[6])
    return R.round_to(np.random.default_rng(R.case_seed(case) + 1).standard_normal((l_out, case[2])).astype(np.float32), dtype)


@pytest.mark.parametrize("case", EPI_CASES, ids=str)
def test_float32_fused_add_is_the_add_op_bit_for_bit(case):
    from pygpukit_amd.core import from_numpy
    from pygpukit_amd.ops.elementwise import add

    pos = _add_operand(case, "f32")
    fused = _run(case, "f32", activation="gelu", channels_last_out=True, add=_dev(pos, "f32")).to_numpy()
    last = _run(case, "f32", activation="gelu", channels_last_out=True)
    both = from_numpy(np.broadcast_to(pos[None], last.shape).copy())
    np.testing.assert_array_equal(fused.view(np.uint32), add(last, both).to_numpy().view(np.uint32))


def _gelu_op_error(pre64):
    """G of the fused bar: the largest |gelu op - float64 GELU| over this case's float32 pre-activations, from the existing float32
    gelu op at run time."""
    from pygpukit_amd.core import from_numpy
    from pygpukit_amd.ops.nn import gelu

    pre32 = np.ascontiguousarray(pre64, np.float32)
    return float(np.max(np.abs(gelu(from_numpy(pre32)).to_numpy().astype(np.float64) - R.gelu(pre32.astype(np.float64)))))


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("case", EPI_CASES, ids=str)
def test_16bit_fused_gelu_and_add(case, dtype):
    """|gpu - gelu64(conv64)| <= out_eps |ref| + 1.13 (accumulation bar) + G; 1.13 bounds |gelu'|.  The add operand is exact
    in fp32 and joins the reference before the output rounding."""
    _, _, _, conv, acc = _case(case, dtype)
    G = _gelu_op_error(conv)
    ref = R.gelu(conv)
    _assert_within(_host(_run(case, dtype, activation="gelu"), dtype), ref, OUT_EPS[dtype] * np.abs(ref) + 1.13 * acc + G,
                   f"conv1d+gelu {case} {dtype} (G = {G:.2e})")
    pos = _add_operand(case, dtype)
    ref = ref.transpose(0, 2, 1) + pos[None].astype(np.float64)
    got = _host(_run(case, dtype, activation="gelu", channels_last_out=True, add=_dev(pos, dtype)), dtype)
    # one more fp32 rounding, of the sum: 2^-24 |ref|
    _assert_within(got, ref, (OUT_EPS[dtype] + 2.0 ** -24) * np.abs(ref) + 1.13 * acc.transpose(0, 2, 1) + G, f"conv1d+gelu+add {case} {dtype}")


# ---- packed weight, out=, argument checks -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("case", [R.CONV_CASES[1], R.CONV_CASES[7]], ids=str)
def test_packed_weight_gives_the_per_call_pack_bit_for_bit(case, dtype):
    from pygpukit_amd.ops.conv import conv1d_pack_weight

    _, w, _, _, _ = _case(case, dtype)
    packed = conv1d_pack_weight(_dev(w, dtype))
    assert packed.shape == (case[4], -(-case[2] // 64) * 64, -(-case[1] // 32) * 32)
    image = R.from_words(_words(packed, dtype), dtype)
    want = np.zeros(packed.shape, np.float32)
    want[:, :case[2], :case[1]] = w.transpose(2, 0, 1)
    np.testing.assert_array_equal(image, want)
    np.testing.assert_array_equal(_words(_run(case, dtype, packed_weight=packed), dtype), _words(_run(case, dtype), dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_out_is_honoured(dtype):
    from pygpukit_amd.core import from_numpy

    case = R.CONV_CASES[4]
    want = _words(_run(case, dtype), dtype)
    nan = np.full(want.shape, np.nan, np.float32) if dtype == "f32" else np.full(want.shape, 0x7FC0 if dtype == "bf16" else 0x7E00, np.uint16)
    out = from_numpy(nan.view(np.float16) if dtype == "f16" else nan)
    assert _run(case, dtype, out=out) is out
    np.testing.assert_array_equal(_words(out, dtype), want)


def test_bad_shapes_raise_before_the_device_is_touched():
    from pygpukit_amd.ops.conv import conv1d

    x, w, b = (_dev(a, "bf16") for a in R.make_conv_case((1, 8, 8, 9, 3, 1, 0)))
    with pytest.raises(ValueError, match="in_channels"):
        conv1d(x, _dev(np.zeros((8, 7, 3), np.float32), "bf16"), b)
    with pytest.raises(ValueError, match="L_out"):
        conv1d(x, _dev(np.zeros((8, 8, 10), np.float32), "bf16"), b)
    with pytest.raises(ValueError, match="add"):
        conv1d(x, w, b, add=_dev(np.zeros((7, 8), np.float32), "bf16"))
