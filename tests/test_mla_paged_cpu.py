"""Batched MLA decode over a paged latent cache without a GPU: the bar's precondition at the GPU tests' shapes, the host-only plan
and its refusals, the wrappers' checks on stand-in arrays, and the exports."""

from types import SimpleNamespace

import numpy as np
import pytest

from tests import mla_paged_ref as P
from tests import mla_ref as R
from tests.conftest import rel_err


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("q_len,heads", P.OP_SHAPES)
def test_bar_precondition(q_len, heads, dtype):
    """The unavoidable roundings alone (inputs, P before P.V, the output) over the whole batch: under half of the GPU bar of 1e-2."""
    ctxs = P.contexts(q_len, 640)
    q, rows, _, _ = P.case(q_len, heads, 16, ctxs, dtype)
    e = rel_err(P.op(q, rows, ctxs, R.SCALE, R.rounder(dtype)), P.op(q, rows, ctxs, R.SCALE))
    print(f"roundings {e:.3e}")
    assert e <= 5e-3


def test_plan():
    from pygpukit_amd.ops.nn import sdpa_mla_paged_plan

    for q_len, heads in P.OP_SHAPES:
        tiles = -(-q_len * heads // 32)
        assert sdpa_mla_paged_plan(heads, q_len, 6, 64, "bfloat16") == ("mla_paged_mfma", (tiles, 1, 6))
        name, grid = sdpa_mla_paged_plan(heads, q_len, 6, 640, "float16")
        assert name == "mla_paged_mfma" and grid[::2] == (tiles, 6) and grid[1] == 5          # 640 / 128 rows: the chunk floor binds
    assert sdpa_mla_paged_plan(128, 1, 32, 4096, "bfloat16")[1] == (4, 4, 32)                 # 128 workgroups x 4 chunks = 512
    assert sdpa_mla_paged_plan(128, 1, 256, 32768, "bfloat16")[1] == (4, 1, 256)              # the batch fills the chip: no split
    assert sdpa_mla_paged_plan(16, 1, 1, 131072, "bfloat16")[1] == (1, 128, 1)                # one sequence: sdpa_mla_plan's split
    for bad in ((0, 1, 1, 64, "bfloat16"), (129, 1, 1, 64, "bfloat16"), (16, 1, 1, 64, "float32"), (16, 65, 1, 64, "float16"),
                (16, 1, 0, 64, "bfloat16"), (16, 1, 1, 0, "bfloat16")):
        with pytest.raises(ValueError, match="pgk_sdpa_mla_paged_plan"):
            sdpa_mla_paged_plan(*bad)


SPEC = dict(q=((3, 1, 16, 576), "bf"), cache=((8, 16, 576), "bf"), out=((3, 1, 16, 512), "bf"), tables=((3, 4), "i32"), lens=((3,), "i32"),
            kv_a=((3, 576), "bf"), gamma=((512,), "bf"), cos=((64, 64), "f32"), pos=((3,), "i32"), slots=((3,), "i32"))
CHECKS = [("sdpa", dict(q=((3, 1, 16, 512), "bf")), 0.07, "q must be"), ("sdpa", dict(q=((1, 16, 576), "bf")), 0.07, "q must be"),
          ("sdpa", dict(cache=((128, 576), "bf")), 0.07, "cache must be"), ("sdpa", dict(cache=((8, 16, 576), "f16")), 0.07, "cache must be"),
          ("sdpa", dict(out=((3, 1, 16, 576), "bf")), 0.07, "out must be"), ("sdpa", dict(tables=((3, 4), "f32")), 0.07, "block_tables must be"),
          ("sdpa", dict(tables=((2, 4), "i32")), 0.07, "block_tables must be"), ("sdpa", dict(lens=((4,), "i32")), 0.07, "context_lens must be"),
          ("sdpa", dict(), 0.0, "scale must be positive"), ("sdpa", dict(), -1.0, "scale must be positive"),
          ("sdpa", dict(q=((3, 1, 129, 576), "bf"), out=((3, 1, 129, 512), "bf")), 0.07, "1 <= H <= 128"),
          ("sdpa", dict(q=((3, 65, 16, 576), "bf"), out=((3, 65, 16, 512), "bf")), 0.07, "q_len <= max_context"),
          ("write", dict(kv_a=((3, 512), "bf")), 0.07, "kv_a must be"), ("write", dict(cache=((8, 16, 576), "f16")), 0.07, "cache must be"),
          ("write", dict(cache=((128, 576), "bf")), 0.07, "cache must be"), ("write", dict(gamma=((512,), "f16")), 0.07, "gamma must be"),
          ("write", dict(cos=((64, 32), "f32")), 0.07, "cos / sin must be"), ("write", dict(pos=((2,), "i32")), 0.07, "positions must be"),
          ("write", dict(slots=((3,), "f32")), 0.07, "slot_mapping must be")]


@pytest.mark.parametrize("op,change,scale,match", CHECKS)
def test_wrappers_check_before_any_launch(op, change, scale, match):
    """Wrong widths, ranks, dtypes and batch sizes, and a non-positive scale, are ValueErrors without a device."""
    from pygpukit_amd.core.dtypes import bfloat16, float16, float32, int32
    from pygpukit_amd.ops.nn import mla

    dt = {"bf": bfloat16, "f16": float16, "f32": float32, "i32": int32}
    a = {n: SimpleNamespace(shape=s, ndim=len(s), dtype=dt[d], size=int(np.prod(s))) for n, (s, d) in {**SPEC, **change}.items()}
    with pytest.raises(ValueError, match=match):
        if op == "sdpa":
            mla.sdpa_mla_paged(a["q"], a["cache"], a["tables"], a["lens"], a["out"], 64, scale)
        else:
            mla.mla_reshape_and_cache(a["kv_a"], a["gamma"], a["cos"], a["cos"], a["pos"], a["cache"], a["slots"])


def test_exports():
    import pygpukit_amd as pk
    from pygpukit_amd import _hip, ops
    from pygpukit_amd.llm.layers import MLAttention
    from pygpukit_amd.ops import nn

    for name in ("allocate_mla_cache", "mla_reshape_and_cache", "sdpa_mla_paged", "sdpa_mla_paged_plan"):
        assert getattr(pk, name) is getattr(ops, name) is getattr(nn, name) and name in nn.__all__ and name in ops.__all__, name
    assert {"pgk_mla_paged_cache_write", "pgk_sdpa_mla_paged", "pgk_sdpa_mla_paged_workspace_bytes", "pgk_sdpa_mla_paged_plan"} <= set(_hip.EXPORTED_SYMBOLS)
    assert len(set(nn.__all__)) == len(nn.__all__) and callable(MLAttention.forward_paged)
    with pytest.raises(ValueError, match="allocate_mla_cache"):
        nn.allocate_mla_cache(4, 0, "bfloat16")
