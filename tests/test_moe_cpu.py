"""CPU tests of the Mixture-of-Experts support: checkpoint detection, config.json parsing, rejection of the MoE
variants MoELayer does not cover, and the restated oracle's routing (tests/moe_ref.py) against plain loops."""

from __future__ import annotations

import json

import numpy as np
import pytest

from tests import moe_ref as R

from pygpukit_amd.llm.config import MIXTRAL_SPEC, MOE_MODEL_SPECS, QWEN3_MOE_SPEC, detect_model_spec
from pygpukit_amd.llm.loader import _moe_fields, _read_config

ATTN = ["model.embed_tokens.weight", "model.layers.0.input_layernorm.weight", "model.layers.0.self_attn.q_proj.weight"]


def test_mixtral_names_detected():
    names = ATTN + ["model.layers.0.block_sparse_moe.gate.weight", "model.layers.0.block_sparse_moe.experts.0.w1.weight"]
    spec = detect_model_spec(names)
    assert spec is MIXTRAL_SPEC and spec.is_moe and MOE_MODEL_SPECS["mixtral"] is spec
    assert spec.moe_gate.format(layer=3) == "model.layers.3.block_sparse_moe.gate.weight"
    assert spec.expert_gate_proj.format(layer=1, expert=7) == "model.layers.1.block_sparse_moe.experts.7.w1.weight"
    assert spec.expert_up_proj.format(layer=1, expert=7) == "model.layers.1.block_sparse_moe.experts.7.w3.weight"
    assert spec.expert_down_proj.format(layer=1, expert=7) == "model.layers.1.block_sparse_moe.experts.7.w2.weight"
    assert spec.gate_proj is None and not spec.use_qk_norm and spec.default_rope_theta == 1e6


def test_qwen3_moe_names_detected():
    names = ATTN + ["model.layers.0.self_attn.q_norm.weight", "model.layers.0.mlp.gate.weight",
                    "model.layers.0.mlp.experts.0.gate_proj.weight"]
    spec = detect_model_spec(names)
    assert spec is QWEN3_MOE_SPEC and spec.is_moe and spec.use_qk_norm and MOE_MODEL_SPECS["qwen3_moe"] is spec
    assert spec.moe_gate.format(layer=0) == "model.layers.0.mlp.gate.weight"
    assert spec.expert_down_proj.format(layer=2, expert=5) == "model.layers.2.mlp.experts.5.down_proj.weight"
    assert spec.default_rope_theta == 1e7


def test_moe_without_qk_norm_rejected():
    with pytest.raises(ValueError, match="only Mixtral and Qwen3-MoE"):
        detect_model_spec(ATTN + ["model.layers.0.mlp.experts.0.gate_proj.weight"])


def _write(tmp_path, conf):
    (tmp_path / "config.json").write_text(json.dumps(conf))
    return _read_config(str(tmp_path / "model.safetensors"))


def test_config_fields_parsed(tmp_path):
    q = _write(tmp_path, {"num_experts": 128, "num_experts_per_tok": 8, "moe_intermediate_size": 768,
                          "intermediate_size": 6144, "norm_topk_prob": True, "decoder_sparse_step": 1, "mlp_only_layers": []})
    assert _moe_fields(QWEN3_MOE_SPEC, q, set()) == dict(num_experts=128, num_experts_per_tok=8, moe_intermediate_size=768)
    m = _write(tmp_path, {"num_local_experts": 8, "num_experts_per_tok": 2, "intermediate_size": 14336})
    assert _moe_fields(MIXTRAL_SPEC, m, set()) == dict(num_experts=8, num_experts_per_tok=2, moe_intermediate_size=14336)


@pytest.mark.parametrize("extra, names, msg", [
    ({"shared_expert_intermediate_size": 512}, set(), "shared experts"),
    ({}, {"model.layers.0.mlp.shared_expert.gate_proj.weight"}, "shared experts"),
    ({"mlp_only_layers": [0]}, set(), "mlp_only_layers"),
    ({"decoder_sparse_step": 2}, set(), "decoder_sparse_step"),
    ({"norm_topk_prob": False}, set(), "norm_topk_prob"),
])
def test_unsupported_variants_rejected(tmp_path, extra, names, msg):
    conf = _write(tmp_path, dict({"num_experts": 8, "num_experts_per_tok": 2, "moe_intermediate_size": 128}, **extra))
    with pytest.raises(ValueError, match=msg):
        _moe_fields(QWEN3_MOE_SPEC, conf, names)


def test_missing_expert_count_rejected(tmp_path):
    with pytest.raises(ValueError, match="num_experts_per_tok"):
        _moe_fields(MIXTRAL_SPEC, _write(tmp_path, {"intermediate_size": 64}), set())


@pytest.mark.parametrize("T, k, E", [(1, 1, 8), (7, 2, 8), (300, 8, 128), (50, 2, 3), (1100, 8, 256)])
def test_oracle_permutation_equals_loop(T, k, E):
    rng = np.random.default_rng(T + E)
    idx = rng.integers(0, E, (T, k)).astype(np.int32)
    idx[: T // 3, 0] = 0                                   # one heavily loaded expert
    if T > 4:
        idx[1, -1] = -1                                    # ids outside [0, E) are not placed
        idx[2, 0] = E
    got = R.permutation(idx, E)
    want = R.permutation_loop(idx, E)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    counts, offsets, perm, rev = got
    placed = perm[: offsets[-1]]
    for e in range(E):                                     # stable: ascending flat index within each expert
        seg = placed[offsets[e]:offsets[e + 1]]
        assert np.all(np.diff(seg) > 0) and np.all(idx.ravel()[seg] == e)
    assert np.all(rev[placed] == np.arange(offsets[-1]))


def test_oracle_topk_ties_and_softmax():
    logits = np.array([[1.0, 3.0, 3.0, 2.0, 3.0], [np.nan, 0.5, 0.5, -np.inf, 0.5]], np.float32)
    w, idx = R.topk_softmax(logits, 3, bf16=False)
    np.testing.assert_array_equal(idx, [[1, 2, 4], [1, 2, 4]])
    np.testing.assert_allclose(w, np.full((2, 3), 1 / 3, np.float32), rtol=1e-6)
    table = R.tile_table(np.array([0, 130, 130, 131], np.int32), 131, 1, 3)
    np.testing.assert_array_equal(table, [[0, 0], [0, 128], [2, 130], [-1, 0], [-1, 0]])
