"""CPU checks of the Llama-4 work: the NumPy restatement (tests/llama4_ref.py) reproduces what the reference's CPU path
recorded in tests/golden/g7_llama4.npz, the public names exist, the config reader and the temperature's step
boundaries."""

from __future__ import annotations

import functools
import json

import numpy as np
import pytest

from tests import llama4_ref as R
from tests.conftest import load_golden

TOL = 1e-5


@functools.lru_cache(maxsize=None)
def _g7():
    return load_golden("g7_llama4.npz")


def _close(got, want):
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape
    err = np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-30)
    assert err <= TOL, err


@pytest.mark.parametrize("tag,shape", [("a", (6, 128)), ("b", (3, 5, 40))])
def test_restated_l2norm_reproduces_the_reference(tag, shape):
    g = _g7()
    assert g[f"l2norm_{tag}_x"].shape == shape
    _close(R.l2norm(g[f"l2norm_{tag}_x"], float(g[f"l2norm_{tag}_eps"])), g[f"l2norm_{tag}_y"])


def test_restated_irope_scale_q_reproduces_the_reference():
    g = _g7()
    a, f = g["scale_q_params"]
    assert g["scale_q_q"].shape == (9, 2, 8) and f == 2.0
    got = R.irope_scale_q(g["scale_q_q"], g["scale_q_pos"], float(a), float(f))
    _close(got, g["scale_q_y"])
    assert len(set(R.irope_temperature(g["scale_q_pos"], float(a), float(f)).tolist())) >= 4      # the scaling really varies


@pytest.mark.parametrize("tag,shape,offset", [("a", (4, 2, 40, 40, 64), 0), ("b", (2, 2, 12, 30, 128), 18)])
def test_restated_sdpa_irope_reproduces_the_reference(tag, shape, offset):
    g = _g7()
    q, k, v, pos = (g[f"sdpa_{tag}_{n}"] for n in ("q", "k", "v", "pos"))
    a, f, off = g[f"sdpa_{tag}_params"]
    assert (q.shape[0], k.shape[0], q.shape[1], k.shape[1], q.shape[2]) == shape and off == offset
    assert pos[0] == offset and (a, f) == (0.5, 16.0)
    _close(R.sdpa_irope(q, k, v, pos, float(a), float(f), int(off)), g[f"sdpa_{tag}_y"])


@functools.lru_cache(maxsize=None)
def _tiny():
    g = _g7()
    return R.make_llama4_weights(R.TINY_CFG, int(g["model_seed"]))


def test_weight_checksum_matches():
    assert abs(R.checksum(_tiny()) - float(_g7()["model_weight_checksum"])) <= 1e-9 * 1e4


def test_restated_model_reproduces_logits_and_greedy_tokens():
    g = _g7()
    prompt = g["model_prompt"]
    assert prompt.shape == (12,) and g["model_tokens"].shape == (6,) and float(g["model_min_gap"]) >= 5e-2
    ids, rows = R.generate(R.TINY_CFG, _tiny(), prompt, 6)
    np.testing.assert_array_equal(ids[12:], g["model_tokens"])
    _close(R.forward(R.TINY_CFG, _tiny(), prompt), g["model_logits"])
    # the margin the GPU test relies on: top-1 minus top-2 of every generated step >= 5e-2 * max|logit|
    for r in rows:
        top = np.sort(r)
        assert top[-1] - top[-2] >= 5e-2 * np.abs(r).max()
    # the temperature changes inside the prompt (floor_scale 4 over 12 positions)
    assert len(set(R.irope_temperature(np.arange(12), R.TINY_CFG["attn_scale"], R.TINY_CFG["floor_scale"]).tolist())) == 4


# ---- public surface (these fail without the feature) -------------------------------------------------------------------

def test_ops_are_exported_from_ops_nn():
    import pygpukit_amd.ops.nn as nn

    for name in ("l2norm", "irope_scale_q", "sdpa_irope", "sdpa_irope_strided"):
        assert callable(getattr(nn, name)), name
        assert name in nn.__all__, name


def test_model_module_exposes_the_reference_names():
    from pygpukit_amd.llm.models import llama4

    for name in ("Llama4Config", "Llama4Attention", "Llama4MLP", "Llama4Block", "Llama4Model", "generate"):
        assert hasattr(llama4, name), name


def test_library_exports_the_llama4_entries():
    from pygpukit_amd import _hip

    lib = _hip.load()
    for name in ("pgk_l2norm", "pgk_irope_scale_q", "pgk_sdpa_irope"):
        assert hasattr(lib, name), name
        assert name in _hip.EXPORTED_SYMBOLS


def test_config_from_json_nested_and_flat(tmp_path):
    from pygpukit_amd.llm.models.llama4 import Llama4Config

    text = {"vocab_size": 100, "hidden_size": 256, "num_hidden_layers": 2, "attn_scale": 0.5, "floor_scale": 4.0,
            "no_rope_layers": [1, 0], "use_qk_norm": False}
    nested, flat = tmp_path / "nested.json", tmp_path / "flat.json"
    nested.write_text(json.dumps({"model_type": "llama4", "vocab_size": 7, "text_config": text}))
    flat.write_text(json.dumps(text))
    for path in (nested, flat):
        c = Llama4Config.from_json(path)
        assert (c.vocab_size, c.hidden_size, c.num_hidden_layers, c.attn_scale, c.floor_scale) == (100, 256, 2, 0.5, 4.0)
        assert c.no_rope_layers == [1, 0] and c.use_qk_norm is False
        # the reference's defaults for what the file leaves out
        assert (c.intermediate_size, c.num_attention_heads, c.num_key_value_heads, c.head_dim) == (8192, 40, 8, 128)
        assert (c.rms_norm_eps, c.max_position_embeddings) == (1e-5, 10485760)
    d = Llama4Config()
    assert (d.vocab_size, d.attn_scale, d.floor_scale, d.use_qk_norm, d.no_rope_layers) == (202048, 0.1, 8192.0, True, None)


@pytest.mark.parametrize("floor_scale", [4.0, 3.0, 8192.0])
def test_temperature_is_exact_at_the_step_boundaries(floor_scale):
    """pos + 1 = k * floor_scale is the first position of step k; the position before it still has step k - 1."""
    a = np.float32(0.1)
    ks = np.arange(1, 40, dtype=np.int64)
    first = ks * int(floor_scale) - 1                     # pos with pos + 1 = k * floor_scale
    want = lambda k: (np.log1p(k.astype(np.float64)).astype(np.float32) * a + np.float32(1)).astype(np.float32)   # noqa: E731
    np.testing.assert_array_equal(R.irope_temperature(first, 0.1, floor_scale), want(ks))
    np.testing.assert_array_equal(R.irope_temperature(first - 1, 0.1, floor_scale), want(ks - 1))
    assert R.irope_temperature([0], 0.1, floor_scale)[0] == (np.float32(1.0) if floor_scale > 1 else want(np.array([1]))[0])
    assert R.irope_temperature(first, 0.1, floor_scale).dtype == np.float32
