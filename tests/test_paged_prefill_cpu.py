"""Host side of paged_attention_prefill: the grid and the refusals of paged_prefill_plan, the wrapper's shape and dtype checks (they
run before anything touches a device, so plain stand-ins for the arrays do), and the oracle's mask rule.  No GPU."""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest

from tests import paged_prefill_ref as P


@pytest.mark.parametrize("heads,tiles", [((2, 2), 2), ((4, 2), 3), ((8, 2), 5), ((8, 1), 9)], ids=["G1", "G2", "G4", "G8"])
def test_plan_grid_packs_the_group_into_the_column_tile(heads, tiles):
    """A column is a (position, head of the group) pair, 128 to a tile: 130 positions are ceil(130 G / 128) tiles."""
    from pygpukit_amd.ops.paged import paged_prefill_plan

    for dtype, d in (("bfloat16", 128), ("float16", 64)):
        assert paged_prefill_plan(9, 130, *heads, d, dtype) == ("paged_prefill_mfma", (tiles, heads[1], 9))
    assert paged_prefill_plan(9, 1, *heads, 128, "bfloat16")[1][0] == 1      # a decode-only step: one tile of G columns
    assert paged_prefill_plan(9, 0, *heads, 128, "bfloat16")[1][0] == 0


@pytest.mark.parametrize("args,why", [((4, 2, 128, "float32"), "bfloat16 / float16 only"), ((4, 2, 96, "bfloat16"), "head_dim"),
                                      ((6, 2, 128, "bfloat16"), "query heads per kv head"), ((5, 2, 128, "float16"), "multiple")],
                         ids=["float32", "D96", "G3", "ragged_heads"])
def test_plan_refuses_what_has_no_kernel(args, why):
    from pygpukit_amd.ops.paged import paged_prefill_plan

    reason, grid = paged_prefill_plan(2, 64, *args)
    assert grid is None and "pgk_paged_attention_prefill" in reason and why in reason


def _arr(shape, dtype):
    return SimpleNamespace(shape=tuple(shape), ndim=len(shape), dtype=dtype, size=int(np.prod(shape)))


@pytest.mark.parametrize("change,match", [
    (dict(q=((10, 4, 64), "bf")), "does not match the cache"), (dict(q=((10, 4, 128), "f16")), "does not match the cache"),
    (dict(v=((6, 2, 16, 64), "bf")), "matching"), (dict(k=((6, 2, 16, 128), "f32"), v=((6, 2, 16, 128), "f32")), "cache dtype"),
    (dict(tables=((12,), "i32")), "block_tables"), (dict(ctx=((3,), "bf")), "context_lens"), (dict(ctx=((4,), "i32")), "context_lens"),
    (dict(cu=((3,), "i32")), "cu_seqlens_q"), (dict(kw=dict(max_query_len=11)), "max_query_len"),
    (dict(q=((10, 6, 128), "bf")), "query heads per kv head"),
], ids=["q_dim", "q_dtype", "v_shape", "cache_f32", "tables_1d", "ctx_dtype", "ctx_size", "cu_size", "max_query_len", "G3"])
def test_wrapper_checks_shapes_and_dtypes(change, match):
    from pygpukit_amd.core.dtypes import bfloat16, float16, float32, int32
    from pygpukit_amd.ops.paged import paged_attention_prefill

    dt = {"bf": bfloat16, "f16": float16, "f32": float32, "i32": int32}
    spec = dict(q=((10, 4, 128), "bf"), k=((6, 2, 16, 128), "bf"), v=((6, 2, 16, 128), "bf"), tables=((3, 4), "i32"), ctx=((3,), "i32"),
                cu=((4,), "i32"), kw={})
    spec.update(change)
    a = {n: _arr(s[0], dt[s[1]]) for n, s in spec.items() if n != "kw"}
    with pytest.raises(ValueError, match=match):
        paged_attention_prefill(a["q"], a["k"], a["v"], a["tables"], a["ctx"], a["cu"], **spec["kw"])


def test_oracle_mask_rule():
    """One page, V rows = one-hot of their position, Q = 0 (uniform weights): row i averages keys 0 .. ctx - q_len + i."""
    v = np.eye(8).reshape(1, 1, 8, 8)
    out = P.paged_attention_prefill(np.zeros((4, 1, 8)), np.zeros((1, 1, 8, 8)), v, np.zeros((2, 1), np.int32), [6, 0], [0, 3, 4])
    for i in range(3):
        n = 6 - 3 + i + 1
        np.testing.assert_allclose(out[i, 0], np.r_[np.full(n, 1.0 / n), np.zeros(8 - n)])
    assert not out[3].any()             # ctx == 0: no visible key
