"""CPU-only checks of the sdpa_causal_fp8 surface and of its restated oracle (tests/fp8_attn_ref.py)."""

from __future__ import annotations

import numpy as np

from oracle import cpu_ref as O
from tests import fp8_attn_ref as R
from tests.conftest import rel_err


def test_library_exports_the_fp8_attention_symbols():
    from pygpukit_amd import _hip

    lib = _hip.load()
    for name in ("pgk_sdpa_causal_fp8", "pgk_quantize_fp8_per_head", "pgk_device_arch"):
        assert hasattr(lib, name), name
        assert name in _hip.EXPORTED_SYMBOLS


def test_python_surface_is_exported_at_every_level():
    import pygpukit_amd as pk

    for mod in (pk.ops.nn, pk.ops, pk):
        for name in ("sdpa_causal_fp8", "fa3_fp8_available", "get_sm_version"):
            assert callable(getattr(mod, name)), (mod.__name__, name)
    for name in ("sdpa_causal_fp8_strided", "quantize_fp8_per_head"):
        assert callable(getattr(pk.ops, name)) and callable(getattr(pk.ops.nn, name))
    assert not hasattr(pk.ops.nn, "test_fp8_mma_direct")


def test_fa3_fp8_available_is_false_without_a_device():
    import pygpukit_amd as pk
    from pygpukit_amd import _hip

    if _hip.device_count() > 0:
        assert pk.fa3_fp8_available() is (pk.get_sm_version() == 950)
    else:
        assert pk.fa3_fp8_available() is False


def test_restatement_exact_integer_case_equals_the_unquantised_oracle():
    """Integers in [-15, 15] are 4-bit significands: the head exponent is -4 and every code decodes to its input, so the
    fp8 restatement IS the unquantised attention."""
    rng = np.random.default_rng(11)
    q, k, v = R.exact_integer_qk(rng, 2, 1, 150, 150)
    for x in (q, k):
        codes, sb = R.quantize_per_head(x)
        assert (sb == 127 - 4).all()
        np.testing.assert_array_equal(R.dequantize_per_head(codes, sb), x.astype(np.float64))
    got, want = R.sdpa_causal_fp8(q, k, v, 1.0 / 256), R.sdpa_causal_unquantised(q, k, v, 1.0 / 256)
    assert rel_err(got, want) == 0.0


def test_restatement_gap_to_the_unquantised_oracle():
    """What makes the GPU comparison discriminating: on normal data the fp8 contract differs from the unquantised op by
    3.05e-2 (measured), three times the 1e-2 bar the kernel must meet against the restatement."""
    rng = np.random.default_rng(0)
    q, k, v = (R.bf16_normal(rng, (4, 200, 128)) for _ in range(3))
    gap = rel_err(R.sdpa_causal_fp8(q, k, v), R.sdpa_causal_unquantised(q, k, v))
    print(f"fp8 restatement vs unquantised oracle: rel_err {gap:.3e}")
    assert gap >= 2e-2


def test_quantiser_restatement_scale_bytes():
    above = lambda a: float(O.bf16_bits_to_f32(O.f32_to_bf16_bits(np.float32([a])) + np.uint16(1))[0])   # noqa: E731
    heads, want = [], []
    for n in (-10, -1, 0, 1, 9):
        a = 448.0 * 2.0 ** n
        for amax, e in ((a, n), (above(a), n + 1)):
            x = np.zeros((7, 128), np.float32)
            x[3, 5], x[1, 100] = -amax, amax / 3
            heads.append(x)
            want.append(e + 127)
    heads.append(np.zeros((7, 128), np.float32))
    want.append(127)
    x = O.bf16_round(np.stack(heads))
    codes, sb = R.quantize_per_head(x)
    np.testing.assert_array_equal(sb, np.uint8(want))
    assert not codes[-1].any()
    # absmax = 448 * 2^n sits exactly on the largest code; one bf16 step above rounds back onto 224 * 2^(n+1)
    assert (codes[0:-1:2, 3, 5] == 0xFE).all() and (codes[1:-1:2, 3, 5] == 0xF6).all()
    assert R.head_exponent(15.0) == -4 and R.head_exponent(2.0 ** 140) == 127 and R.head_exponent(2.0 ** -140) == -127
