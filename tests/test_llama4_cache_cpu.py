"""CPU checks of the Llama-4 KV-cache work: the cached restatement (tests/llama4_cache_ref.py) reproduces the uncached
one (tests/llama4_ref.forward) row for row, whatever the chunking, and the public names exist.

Bar 1e-9 (rel_err, float64 on both sides): the two differ only in the order rows are computed in - a cached row sums
over exactly the keys the causal mask leaves it in the full forward - so the difference is float64 summation noise."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from tests import llama4_cache_ref as C
from tests import llama4_ref as R
from tests.conftest import load_golden, rel_err

TOL = 1e-9
PROMPT, STEPS = 12, 24


@functools.lru_cache(maxsize=None)
def _sequence():
    """(weights, the g7 prompt followed by 24 greedy tokens of the restatement, R.forward on those 36 tokens)."""
    g = load_golden("g7_llama4.npz")
    w = R.make_llama4_weights(R.TINY_CFG, int(g["model_seed"]))
    ids, _ = R.generate(R.TINY_CFG, w, g["model_prompt"], STEPS)
    ids = ids[:PROMPT + STEPS]
    np.testing.assert_array_equal(ids[PROMPT:PROMPT + 6], g["model_tokens"])
    full = R.forward(R.TINY_CFG, w, ids)
    ids.setflags(write=False)
    full.setflags(write=False)
    return w, ids, full


@pytest.mark.parametrize("chunks", [[12], [5, 7]])
def test_cached_restatement_reproduces_the_full_forward(chunks):
    w, ids, full = _sequence()
    got = C.teacher_forced(R.TINY_CFG, w, ids, PROMPT, chunks)
    assert got.shape == full.shape == (PROMPT + STEPS, R.TINY_CFG["vocab_size"])
    for name, rows in (("prefill", slice(0, PROMPT)), ("steps", slice(PROMPT, PROMPT + STEPS))):
        err = rel_err(got[rows], full[rows])
        print(f"chunks {chunks} {name}: rel_err {err:.3e}")
        assert err <= TOL, name
    # the temperature steps inside the decoded range (floor_scale 4: positions 15, 19, ..., 35)
    t = R.irope_temperature(np.arange(PROMPT, PROMPT + STEPS), R.TINY_CFG["attn_scale"], R.TINY_CFG["floor_scale"])
    assert len(set(t.tolist())) == 7


def test_cached_restatement_refuses_rows_out_of_order():
    w, ids, _ = _sequence()
    m = C.CachedLlama4(R.TINY_CFG, w)
    m.prefill(ids[:3], 0)
    with pytest.raises(ValueError):
        m.step(ids[3], 5)


# ---- public surface (these fail without the feature) -------------------------------------------------------------------

def test_library_exports_the_cached_decode_entries():
    from pygpukit_amd import _hip

    lib = _hip.load()
    for name in ("pgk_llama4_qk_norm_cache_write", "pgk_sdpa_irope_fixed_cache"):
        assert hasattr(lib, name), name
        assert name in _hip.EXPORTED_SYMBOLS


def test_cached_decode_ops_are_exported_from_ops_nn():
    import pygpukit_amd.ops.nn as nn

    for name in ("llama4_qk_norm_cache_write", "llama4_qk_norm_cache_write_ptr", "sdpa_irope_fixed_cache", "sdpa_irope_fixed_cache_ptr"):
        assert callable(getattr(nn, name)), name
        assert name in nn.__all__, name


def test_model_has_the_cached_decode_methods():
    import inspect

    from pygpukit_amd.llm.models import llama4

    for name in ("init_fixed_cache", "prefill_fixed_cache", "decode_step", "capture_decode", "decode_step_graph"):
        assert callable(getattr(llama4.Llama4Model, name)), name
    p = inspect.signature(llama4.generate).parameters
    assert p["use_cache"].default is False and p["use_graph"].default is False          # the uncached loop stays the default
