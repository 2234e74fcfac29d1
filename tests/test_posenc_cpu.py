"""CPU tests of the positional-encoding family: the NumPy restatement (tests/posenc_ref.py) against what the reference's CPU
path returned (tests/golden/g8_posenc.npz), the host halves of the table builders against both, the exported C ABI and the
Python surface.  Everything here is bit-exact: the tables are host arithmetic in the reference's operation order."""

from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

from tests import posenc_ref as P
from tests.conftest import load_golden

TABLE_SHAPES = ((64, 16, 10000.0), (70, 40, 500000.0), (300, 128, 10000.0))
SCALES = (1.0, 2.0, 4.0)
NEW_SYMBOLS = ("pgk_pope_inplace", "pgk_alibi_compute_bias", "pgk_alibi_add_bias", "pgk_sdpa_alibi", "pgk_sdpa_alibi_fixed_cache")
NEW_NAMES = ("rope_init_ntk_aware", "rope_init_yarn", "rope_init_linear", "pope_init_encoding", "pope_inplace", "alibi_init_slopes",
             "alibi_compute_bias", "alibi_add_bias", "sdpa_alibi", "sdpa_alibi_strided", "sdpa_alibi_fixed_cache",
             "sdpa_alibi_fixed_cache_ptr")


@functools.lru_cache(maxsize=None)
def _g():
    return load_golden("g8_posenc.npz")


def _ref_table(kind, S, D, base, scale, **kw):
    if kind == "yarn":
        return P.rope_init_yarn(S, D, base, scale, original_max_len=int(_g()["yarn_original_max_len"]), **kw)
    return {"ntk": P.rope_init_ntk_aware, "linear": P.rope_init_linear}[kind](S, D, base, scale, **kw)


def _host_table(kind, S, D, base, scale, **kw):
    from pygpukit_amd.ops.nn import rope as R

    if kind == "yarn":
        return R.rope_init_yarn_host(S, D, base, scale, original_max_len=int(_g()["yarn_original_max_len"]), **kw)
    return {"ntk": R.rope_init_ntk_aware_host, "linear": R.rope_init_linear_host}[kind](S, D, base, scale, **kw)


@pytest.mark.parametrize("kind", ["ntk", "linear", "yarn"])
@pytest.mark.parametrize("S,D,base", TABLE_SHAPES)
def test_rope_tables_equal_the_reference_cpu_path(kind, S, D, base):
    g = _g()
    rows = g[f"rows_{S}"]
    for scale in SCALES:
        tag = f"{S}_{D}_{int(scale)}"
        kw = {"mscale": 0.0} if kind == "yarn" else {}          # the reference's CPU path drops mscale
        for tables in (_ref_table(kind, S, D, base, scale, **kw), _host_table(kind, S, D, base, scale, **kw)):
            for t, name in zip(tables, ("cos", "sin")):
                assert t.dtype == np.float32 and t.shape == (S, D)
                np.testing.assert_array_equal(t[rows], g[f"{kind}_{name}_{tag}"], err_msg=f"{kind} {name} {tag}")


def test_scaling_changes_the_tables():
    g = _g()
    for kind in ("ntk", "linear", "yarn"):
        assert not np.array_equal(g[f"{kind}_cos_300_128_1"], g[f"{kind}_cos_300_128_4"])
    np.testing.assert_array_equal(g["ntk_cos_300_128_1"], g["linear_cos_300_128_1"])


def test_yarn_fixture_has_untouched_and_ramped_pairs():
    """original_max_len = 64 at D = 128: 47 pairs keep their frequency (ramp 1) and 17 are ramped towards inv_freq / scale.
    No pair is scaled in full: the shortest wavelength, 2 pi, is already beyond original_max_len / beta_fast = 2."""
    _, ramp = P.yarn_inv_freq(128, 10000.0, 4.0, int(_g()["yarn_original_max_len"]), 32.0, 1.0)
    assert (ramp == 1).sum() == 47 and ((ramp > 0) & (ramp < 1)).sum() == 17
    assert (np.diff(ramp) >= 0).all()          # the SHORT wavelengths (low pair index) are the interpolated ones


@pytest.mark.parametrize("S,D,base", TABLE_SHAPES)
def test_yarn_mscale_follows_the_device_rule(S, D, base):
    from pygpukit_amd.ops.nn import rope as R

    g, orig = _g(), int(_g()["yarn_original_max_len"])
    rows = g[f"rows_{S}"]
    for scale in SCALES:
        f = np.float32(0.1 * np.log(scale) + 1.0)
        assert f == P.yarn_mscale_factor(scale, 0.1)
        for fn in (P.rope_init_yarn, R.rope_init_yarn_host):
            for t, name in zip(fn(S, D, base, scale, original_max_len=orig), ("cos", "sin")):          # default mscale = 0.1
                np.testing.assert_array_equal(t[rows], g[f"yarn_{name}_{S}_{D}_{int(scale)}"] * f)
            for t, name in zip(fn(S, D, base, scale, original_max_len=orig, mscale=0.0), ("cos", "sin")):
                np.testing.assert_array_equal(t[rows], g[f"yarn_{name}_{S}_{D}_{int(scale)}"])
    assert np.float32(0.1 * np.log(4.0) + 1.0) > 1.1


@pytest.mark.parametrize("S,D,theta", [(300, 128, 1e4), (4096, 64, 1e6), (70, 40, 5e5)])
def test_half_layout_of_linear_equals_precompute_freqs_cis(S, D, theta):
    from pygpukit_amd.llm.layers.rope import precompute_freqs_cis
    from pygpukit_amd.ops.nn import rope as R

    want = precompute_freqs_cis(D, S, theta)
    for fn in (R.rope_init_linear_host, P.rope_init_linear):
        for got, w in zip(fn(S, D, theta, 1.0, layout="half"), want):
            assert got.dtype == np.float32
            np.testing.assert_array_equal(got, w)


@pytest.mark.parametrize("kind", ["ntk", "linear", "yarn"])
def test_half_and_interleaved_layouts_hold_the_same_columns(kind):
    for S, D, base in TABLE_SHAPES:
        inter = _host_table(kind, S, D, base, 2.0)
        half = _host_table(kind, S, D, base, 2.0, layout="half")
        for a, b in zip(half, inter):
            np.testing.assert_array_equal(a[:, :D // 2], b[:, 0::2])
            np.testing.assert_array_equal(a[:, D // 2:], b[:, 1::2])
            np.testing.assert_array_equal(b[:, 0::2], b[:, 1::2])


def test_pope_encoding_and_pope_inplace_equal_the_reference():
    from pygpukit_amd.ops.nn import rope as R

    g = _g()
    for fn in (P.pope_init_encoding, R.pope_init_encoding_host):
        np.testing.assert_array_equal(fn(16, 8), g["pope_enc_16_8"])
        np.testing.assert_array_equal(fn(300, 128)[g["rows_300"]], g["pope_enc_300_128"])
    q, k = P.pope_inplace(g["pope_q"], g["pope_k"], g["pope_enc_16_8"], start_pos=2)
    np.testing.assert_array_equal(q, g["pope_q_y"])
    np.testing.assert_array_equal(k, g["pope_k_y"])


def test_alibi_slopes_bias_and_add_bias_equal_the_reference():
    from pygpukit_amd.ops.nn import rope as R

    g = _g()
    for h in (1, 2, 8, 12, 32, 40):
        for fn in (P.alibi_init_slopes, R.alibi_init_slopes_host):
            got = fn(h)
            assert got.dtype == np.float32
            np.testing.assert_array_equal(got, g[f"slopes_{h}"])
    np.testing.assert_array_equal(g["slopes_8"], np.float32(2.0) ** -np.arange(1, 9, dtype=np.float32))
    np.testing.assert_array_equal(P.alibi_compute_bias(5, 8, g["slopes_8"], True), g["bias_5_8_causal"])
    np.testing.assert_array_equal(P.alibi_compute_bias(5, 8, g["slopes_8"], False), g["bias_5_8_full"])
    assert g["bias_5_8_full"][0, 0, 4] == 2.0 and g["bias_5_8_causal"][0, 0, 4] == np.float32(-1e9)
    np.testing.assert_array_equal(P.alibi_add_bias(g["add_bias_scores"], g["slopes_8"], 4), g["add_bias_y"])


def test_restated_attention_equals_attention_over_the_materialised_bias():
    rng = np.random.default_rng(3)
    q, k, v = rng.standard_normal((4, 9, 16)), rng.standard_normal((2, 9, 16)), rng.standard_normal((2, 9, 16))
    slopes = P.alibi_init_slopes(4)
    a = P.sdpa_alibi(q, k, v, slopes)
    b = P.sdpa_with_bias(q, k, v, P.alibi_compute_bias(9, 4, slopes, True))
    np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12)
    # a prefix: the last rows of the full problem
    np.testing.assert_allclose(P.sdpa_alibi(q[:, 5:], k, v, slopes), a[:, 5:], rtol=1e-12, atol=1e-12)


def test_library_exports_and_python_surface():
    from pygpukit_amd import _hip
    from pygpukit_amd.ops import nn

    lib = ctypes.CDLL(_hip.LIB_PATH)
    for sym in NEW_SYMBOLS:
        assert hasattr(lib, sym), sym
        assert sym in _hip.EXPORTED_SYMBOLS
    for name in NEW_NAMES:
        assert name in nn.__all__ and callable(getattr(nn, name)), name
    assert len(set(nn.__all__)) == len(nn.__all__)


def test_host_builders_refuse_bad_arguments():
    from pygpukit_amd.ops.nn import rope as R

    for fn in (R.rope_init_ntk_aware_host, R.rope_init_linear_host, R.rope_init_yarn_host):
        with pytest.raises(ValueError, match="head_dim"):
            fn(8, 7)
        with pytest.raises(ValueError, match="head_dim"):
            fn(8, 0)
        with pytest.raises(ValueError, match="max_seq_len"):
            fn(0, 8)
        with pytest.raises(ValueError, match="scale"):
            fn(8, 8, scale=0.0)
        with pytest.raises(ValueError, match="scale"):
            fn(8, 8, scale=-2.0)
        with pytest.raises(ValueError, match="layout"):
            fn(8, 8, layout="pairs")
        assert fn(8, 8)[0].shape == (8, 8)
    with pytest.raises(ValueError, match="head_dim"):
        R.pope_init_encoding_host(8, 5)
    with pytest.raises(ValueError, match="max_seq_len"):
        R.pope_init_encoding_host(0, 8)
    with pytest.raises(ValueError, match="num_heads"):
        R.alibi_init_slopes_host(0)
