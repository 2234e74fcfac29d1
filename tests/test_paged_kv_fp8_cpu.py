"""Host side of the FP8 paged KV cache: paged_kv_fp8_plan's names, grids, refusals; the wrappers' checks on stand-in arrays.  No GPU."""

from types import SimpleNamespace

import numpy as np
import pytest


@pytest.mark.parametrize("heads,groups,tiles", [((2, 2), 2, 2), ((4, 2), 2, 3), ((8, 2), 2, 5), ((8, 1), 2, 9)], ids=["G1", "G2", "G4", "G8"])
def test_plan_names_and_grids(heads, groups, tiles):
    from pygpukit_amd.ops.paged import paged_kv_fp8_plan, paged_prefill_plan

    for dtype, d in (("bfloat16", 128), ("float16", 64)):
        for max_context, nsplit in ((0, 1), (512, 1), (513, 2), (1536, 3), (1 << 20, 32)):
            assert paged_kv_fp8_plan("decode", 9, max_context, *heads, d, dtype) == ("paged_kv_fp8_split", (nsplit, groups, 9))
        assert paged_kv_fp8_plan("prefill", 9, 130, *heads, d, dtype) == ("paged_kv_fp8_prefill_mfma", (tiles, heads[1], 9))
        assert paged_kv_fp8_plan("prefill", 9, 130, *heads, d, dtype)[1] == paged_prefill_plan(9, 130, *heads, d, dtype)[1]


@pytest.mark.parametrize("op,entry", [("decode", "pgk_paged_attention_v1_fp8"), ("prefill", "pgk_paged_attention_prefill_fp8")])
@pytest.mark.parametrize("args,why", [((4, 2, 128, "float32"), "bfloat16 / float16 only"), ((4, 2, 96, "bfloat16"), "head_dim"),
                                      ((6, 2, 128, "bfloat16"), "query heads per kv head"), ((5, 2, 128, "float16"), "multiple")],
                         ids=["float32", "D96", "G3", "ragged_heads"])
def test_plan_refuses_what_has_no_kernel(args, why, op, entry):
    from pygpukit_amd.ops.paged import paged_kv_fp8_plan

    reason, grid = paged_kv_fp8_plan(op, 2, 64, *args)
    assert grid is None and entry in reason and why in reason


def _arr(shape, dtype):
    return SimpleNamespace(shape=tuple(shape), ndim=len(shape), dtype=dtype, size=int(np.prod(shape)))


SPEC = dict(q=((3, 4, 128), "bf"), kn=((3, 2, 128), "bf"), k=((6, 2, 16, 128), "u8"), v=((6, 2, 16, 128), "u8"), ks=((2,), "f32"),
            vs=((2,), "f32"), tables=((3, 4), "i32"), ctx=((3,), "i32"), cu=((4,), "i32"), slots=((3,), "i32"))

CHECKS = [
    ("cache_bf16", dict(k=((6, 2, 16, 128), "bf"), v=((6, 2, 16, 128), "bf")), "uint8", "decode prefill write"),
    ("v_shape", dict(v=((6, 2, 16, 64), "u8")), "matching uint8", "decode prefill write"),
    ("k_scale_len", dict(ks=((3,), "f32")), "k_scale must be float32", "decode prefill write"),
    ("v_scale_dtype", dict(vs=((2,), "bf")), "v_scale must be float32", "decode prefill write"),
    ("q_dim", dict(q=((3, 4, 64), "bf")), "q .* must be bfloat16 / float16", "decode prefill"),
    ("q_dtype", dict(q=((3, 4, 128), "u8")), "q .* must be bfloat16 / float16", "decode prefill"),
]


@pytest.mark.parametrize("op,change,match", [pytest.param(op, change, match, id=f"{op}-{name}") for name, change, match, ops in CHECKS
                                             for op in ops.split()])
def test_wrappers_check_shapes_and_dtypes(op, change, match):
    from pygpukit_amd.core.dtypes import bfloat16, float32, int32, uint8
    from pygpukit_amd.ops import paged

    dt = {"bf": bfloat16, "f32": float32, "i32": int32, "u8": uint8}
    a = {n: _arr(s[0], dt[s[1]]) for n, s in {**SPEC, **change}.items()}
    with pytest.raises(ValueError, match=match):
        if op == "decode":
            paged.paged_attention_v1_fp8(a["q"], a["k"], a["v"], a["ks"], a["vs"], a["tables"], a["ctx"])
        elif op == "prefill":
            paged.paged_attention_prefill_fp8(a["q"], a["k"], a["v"], a["ks"], a["vs"], a["tables"], a["ctx"], a["cu"])
        else:
            paged.reshape_and_cache_fp8(a["kn"], a["kn"], a["k"], a["v"], a["slots"], a["ks"], a["vs"])


def test_the_16_bit_ops_still_refuse_uint8_caches():
    from pygpukit_amd.core.dtypes import bfloat16, int32, uint8
    from pygpukit_amd.ops import paged

    q, c, i = _arr((3, 4, 128), bfloat16), _arr((6, 2, 16, 128), uint8), lambda *s: _arr(s, int32)
    for run in (lambda: paged.paged_attention_v1(q, c, c, i(3, 4), i(3)), lambda: paged.paged_attention_prefill(q, c, c, i(3, 4), i(3), i(4)),
                lambda: paged.reshape_and_cache(_arr((3, 2, 128), bfloat16), _arr((3, 2, 128), bfloat16), c, c, i(3))):
        with pytest.raises(ValueError, match="cache dtype must be float16 or bfloat16"):
            run()
