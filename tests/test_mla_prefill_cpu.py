"""sdpa_mla_prefill without a GPU: the exports, the host-only plan and its refusals, and the precondition of the GPU tests' bar."""

from types import SimpleNamespace

import pytest

from tests import mla_prefill_ref as P
from tests import mla_ref as R
from tests.conftest import rel_err


def test_exports():
    import pygpukit_amd as pk
    from pygpukit_amd import _hip, ops
    from pygpukit_amd.ops import nn

    for name in ("sdpa_mla_prefill", "sdpa_mla_prefill_plan"):
        assert getattr(pk, name) is getattr(ops, name) is getattr(nn, name) and name in nn.__all__ and name in ops.__all__, name
    assert {"pgk_sdpa_mla_prefill", "pgk_sdpa_mla_prefill_plan"} <= set(_hip.EXPORTED_SYMBOLS)
    assert len(set(nn.__all__)) == len(nn.__all__)


@pytest.mark.parametrize("heads,q_len,kv_len,dtype,tiles", [(1, 1, 1, "bfloat16", 1), (128, 128, 128, "float16", 1), (3, 129, 400, "bfloat16", 2)])
def test_plan(heads, q_len, kv_len, dtype, tiles):
    from pygpukit_amd.ops.nn import sdpa_mla_prefill_plan

    assert sdpa_mla_prefill_plan(heads, q_len, kv_len, dtype) == ("mla_prefill_mfma", (tiles, heads))


@pytest.mark.parametrize("bad", [(0, 1, 1, "bfloat16"), (129, 1, 1, "bfloat16"), (4, 0, 1, "float16"), (4, 5, 4, "float16"), (4, 1, 1, "float32")])
def test_plan_refuses(bad):
    from pygpukit_amd.ops.nn import sdpa_mla_prefill_plan

    with pytest.raises(ValueError, match="pgk_sdpa_mla_prefill_plan"):
        sdpa_mla_prefill_plan(*bad)


def test_layer_refuses_other_head_dims():
    """forward_prefill checks the head dims before it touches the cache or the device: a stand-in for self is enough."""
    from pygpukit_amd.llm.layers import MLAttention

    with pytest.raises(ValueError, match="qk_nope_head_dim = 128"):
        MLAttention.forward_prefill(SimpleNamespace(num_heads=4, qk_nope_head_dim=32, v_head_dim=32), None, 0)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("shape", P.SHAPES)
def test_bar_precondition(shape, dtype):
    """The kernel's unavoidable roundings (inputs, P before P.V, the output) against float64 at every GPU shape: a third of 1e-2."""
    e = rel_err(P.op(*P.case(*shape, dtype), R.SCALE, R.rounder(dtype)), P.exact(*shape, dtype))
    print(f"{shape} {dtype}: {e:.3e}")
    assert e <= 1e-2 / 3
