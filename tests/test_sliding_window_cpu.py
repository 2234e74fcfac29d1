"""Host logic of sliding-window attention: config parsing, layer_types, plan strings, and
the CPU precondition of the GPU tests' reversed staircase.  No GPU."""

from __future__ import annotations

import numpy as np
import pytest

from tests import attn_stair_ref as S
from tests import sliding_window_ref as W


# ---- config --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hf,want", [
    ({"model_type": "mistral", "sliding_window": 4096}, (4096, None)),
    ({"model_type": "mistral", "sliding_window": None}, (None, None)),
    ({"model_type": "llama"}, (None, None)),
    ({"sliding_window": 8, "layer_types": ["sliding_attention", "full_attention"] * 2}, (8, ["sliding_attention", "full_attention"] * 2)),
    ({"sliding_window": 8, "layer_types": ["full_attention"] * 4}, (None, None)),
    ({"model_type": "qwen2", "sliding_window": 32768, "use_sliding_window": False, "max_window_layers": 2}, (None, None)),
    ({"model_type": "qwen2", "sliding_window": 16, "use_sliding_window": True, "max_window_layers": 3},
     (16, ["full_attention"] * 3 + ["sliding_attention"])),
], ids=["mistral", "mistral_null", "llama", "layer_types", "all_full", "qwen2_off", "qwen2_on"])
def test_config_json_to_transformer_config(hf, want):
    from pygpukit_amd.llm.config import TransformerConfig, sliding_window_fields

    cfg = TransformerConfig(num_layers=4, **sliding_window_fields(hf, 4))
    assert (cfg.sliding_window, cfg.layer_types) == want
    windows = [cfg.layer_window(i) for i in range(4)]
    assert windows == [want[0] if want[0] and (want[1] is None or want[1][i] == "sliding_attention") else None for i in range(4)]
    assert cfg.min_window == want[0]


# ---- plans ------------------------------------------------------------------------------------------------------------------------
def test_plan_splits_by_the_band_not_by_kv_len(monkeypatch):
    """With no device the planner assumes 256 CUs.  2 heads x 6 query tiles: the band of W = 400 is 527 keys = 9 tiles -> two runs,
    where the 700 keys of the causal triangle (11 tiles) give two as well and a band of 300 (427 keys, 7 tiles) none."""
    from pygpukit_amd.ops.nn import sdpa_window_plan

    monkeypatch.delenv("PYGPUKIT_FLASH_ATTENTION", raising=False)
    assert sdpa_window_plan(2, 1, 700, 700, 64, 400, "bfloat16") == ("window_flash", 2)
    assert sdpa_window_plan(2, 1, 700, 700, 64, 300, "bfloat16") == ("window_flash", 1)
    assert sdpa_window_plan(2, 1, 700, 8000, 64, 400, "bfloat16") == ("window_flash", 2)      # kv_len does not matter
    assert sdpa_window_plan(2, 1, 700, 8000, 64, 8000, "bfloat16")[1] == 4                     # plain causal: 125 tiles
    for bad in ((2, 1, 0, 10, 64, 4), (3, 2, 5, 10, 64, 4), (2, 1, 11, 10, 64, 4), (2, 1, 5, 10, 64, 0)):
        with pytest.raises(ValueError, match="pgk_sdpa_window_plan"):
            sdpa_window_plan(*bad, "bfloat16")


def test_build_engine_refuses_a_window_smaller_than_the_context():
    from pygpukit_amd.llm.config import TransformerConfig
    from pygpukit_amd.llm.models.causal import CausalTransformerModel

    cfg = TransformerConfig(num_layers=2, sliding_window=48)
    with pytest.raises(NotImplementedError, match="sliding-window"):
        CausalTransformerModel(cfg, None, [], None).build_engine(max_seq_len=256)


# ---- the oracle and the staircase ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(4, 2, 200, 200, 63), (4, 2, 200, 200, 64), (4, 2, 200, 200, 65), (2, 1, 700, 700, 400), (2, 1, 70, 300, 100)],
                         ids=str)
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_staircase_precondition(shape, dtype):
    """Ascending: the oracle returns the V row of the last visible key.  Reversed along the key axis: of the FIRST visible key -
    and a window one key wider returns another row (except where the window already reaches key 0)."""
    hq, hkv, q_len, kv_len, window = shape
    st = S.make_stair(hq, hkv, q_len, kv_len, 64, dtype)
    off, heads = kv_len - q_len, np.arange(hq) // st.rep
    S.check_precondition(W.sdpa_window(st.q, st.k, st.v, window, 1.0), st.expected(off), "ascending")
    k, v = st.k[:, ::-1], st.v[:, ::-1]
    first = np.maximum(off + np.arange(q_len) - window + 1, 0)
    S.check_precondition(W.sdpa_window(st.q, k, v, window, 1.0), v[heads][:, first], "reversed")
    wider = W.sdpa_window(st.q, k, v, window + 1, 1.0)
    moved = first > 0
    assert moved.any() and np.all(np.abs(wider - v[heads][:, first])[:, moved].max(axis=-1) > 1e-3)
