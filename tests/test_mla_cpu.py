"""Multi-head latent attention without a GPU: the absorbed form against the textbook oracle, the bar's precondition, the host-only
plan, the wrappers' checks on stand-in arrays, and the exports."""

from types import SimpleNamespace

import numpy as np
import pytest

from tests import mla_ref as R
from tests.conftest import rel_err


@pytest.mark.parametrize("q_lora", [None, 96])
def test_absorbed_form_is_the_textbook_form(q_lora):
    """float64, to rounding; and the layer with every 16-bit rounding of the absorbed op sequence stays under HALF the GPU bar."""
    w, a = R.make_weights(5, q_lora), (R.LAYER["heads"], R.LAYER["nope"], R.LAYER["v"], R.LAYER_SCALE)
    text, absorbed, rounded = R.Layer(w, *a), R.Layer(w, *a, absorbed=True), R.Layer(w, *a, absorbed=True, rnd=R.rounder("bf16"))
    for x in R.layer_inputs():
        want = text(x)
        assert rel_err(absorbed(x), want) <= 1e-12
        e = rel_err(rounded(x), want)
        print(f"q_lora {q_lora}, rows {x.shape[0]}: bf16 roundings {e:.3e}")
        assert e <= 5e-3


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("q_len,heads,max_seq", R.DECODE_SHAPES + R.MULTI_SHAPES)
def test_bar_precondition(q_len, heads, max_seq, dtype):
    """The op's unavoidable roundings (inputs, P before P.V, the output) against float64, at the GPU tests' shapes: under half of 1e-2."""
    q, cache = R.case(q_len, heads, max_seq, dtype)
    for ctx in (q_len, max_seq):
        e = rel_err(R.op(q, cache, ctx, R.SCALE, R.rounder(dtype)), R.op(q, cache, ctx, R.SCALE))
        print(f"ctx {ctx}: {e:.3e}")
        assert e <= 5e-3


def test_plan():
    from pygpukit_amd.ops.nn import sdpa_mla_plan

    for heads, q_len in ((1, 1), (128, 1), (20, 5)):
        assert sdpa_mla_plan(heads, q_len, 64, "bfloat16") == ("mla_latent_mfma", 32, 1)
        name, cols, chunks = sdpa_mla_plan(heads, q_len, 600, "float16")
        assert (name, cols) == ("mla_latent_mfma", 32) and chunks > 1
    assert sdpa_mla_plan(128, 1, 131072, "bfloat16")[2] * 4 >= 512          # 4 column tiles: the chunks fill 256 CUs twice
    for bad in ((0, 1, 64, "bfloat16"), (129, 1, 64, "bfloat16"), (16, 1, 64, "float32"), (16, 65, 64, "float16")):
        with pytest.raises(ValueError, match="pgk_sdpa_mla_plan"):
            sdpa_mla_plan(*bad)


SPEC = dict(q=((1, 16, 576), "bf"), cache=((64, 576), "bf"), out=((1, 16, 512), "bf"), kv_a=((1, 576), "bf"), gamma=((512,), "bf"),
            cos=((64, 64), "f32"))
CHECKS = [("sdpa", dict(q=((1, 16, 512), "bf")), 0.07, "q must be"), ("sdpa", dict(cache=((64, 512), "bf")), 0.07, "cache must be"),
          ("sdpa", dict(cache=((64, 576), "f16")), 0.07, "cache must be"), ("sdpa", dict(out=((1, 16, 576), "bf")), 0.07, "out must be"),
          ("sdpa", dict(), 0.0, "scale must be positive"), ("sdpa", dict(), -1.0, "scale must be positive"),
          ("sdpa", dict(q=((1, 129, 576), "bf"), out=((1, 129, 512), "bf")), 0.07, "1 <= H <= 128"),
          ("write", dict(kv_a=((1, 512), "bf")), 0.07, "kv_a must be"), ("write", dict(cache=((64, 576), "f16")), 0.07, "cache must be"),
          ("write", dict(gamma=((512,), "f16")), 0.07, "gamma must be"), ("write", dict(cos=((64, 32), "f32")), 0.07, "cos / sin must be")]


@pytest.mark.parametrize("op,change,scale,match", CHECKS)
def test_wrappers_check_before_any_launch(op, change, scale, match):
    """Wrong widths, mismatched dtypes and a non-positive scale are ValueErrors of the host and the _ptr form, without a device."""
    from pygpukit_amd.core.dtypes import bfloat16, float16, float32, int32
    from pygpukit_amd.ops.nn import mla

    dt = {"bf": bfloat16, "f16": float16, "f32": float32, "i32": int32}
    a = {n: SimpleNamespace(shape=s, ndim=len(s), dtype=dt[d], size=int(np.prod(s))) for n, (s, d) in {**SPEC, "buf": ((1,), "i32"), **change}.items()}
    runs = ((lambda: mla.sdpa_mla_fixed_cache(a["q"], a["cache"], a["out"], 8, scale),
             lambda: mla.sdpa_mla_fixed_cache_ptr(a["q"], a["cache"], a["out"], a["buf"], scale)) if op == "sdpa" else
            (lambda: mla.mla_cache_write(a["kv_a"], a["gamma"], a["cos"], a["cos"], a["cache"], 0),
             lambda: mla.mla_cache_write_ptr(a["kv_a"], a["gamma"], a["cos"], a["cos"], a["cache"], a["buf"])))
    for run in runs:
        with pytest.raises(ValueError, match=match):
            run()


def test_exports():
    import pygpukit_amd as pk
    from pygpukit_amd import _hip, ops
    from pygpukit_amd.llm.layers import MLAttention  # noqa: F401
    from pygpukit_amd.ops import nn

    for name in ("mla_cache_write", "mla_cache_write_ptr", "sdpa_mla_fixed_cache", "sdpa_mla_fixed_cache_ptr", "sdpa_mla_plan"):
        assert getattr(pk, name) is getattr(ops, name) is getattr(nn, name) and name in nn.__all__ and name in ops.__all__, name
    assert {"pgk_mla_cache_write", "pgk_sdpa_mla_fixed_cache", "pgk_sdpa_mla_plan", "pgk_sdpa_mla_workspace_bytes"} <= set(_hip.EXPORTED_SYMBOLS)
    assert len(set(nn.__all__)) == len(nn.__all__)
