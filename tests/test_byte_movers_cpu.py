"""CPU side of the byte-mover checks (tests/byte_movers_ref.py, tests/test_byte_movers_gpu.py): for every case of the table

  * tensor_op_plan, the host-side query built from the functions the launchers call (csrc/tensor_plan.h), reports the leaf the
    table names, from the low address bits the case's misaligned operands will have;
  * the table reaches every leaf the query can print for every op that has it, every operand a caller can supply is misaligned
    in some case, and every wrap case has more work items than tensor_op_grid(...) * 256 with no row to spare;
  * the query rejects what the entry points reject;
  * every applicable planted error (PLANTED) changes at least one word of the oracle's output, and every planted error is used.

The ops are exact: nothing here or in the GPU file compares under a tolerance.  Nothing here needs a device."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from pygpukit_amd import _hip, ops
from pygpukit_amd.ops.plan import TENSOR_PLAN_OPS, tensor_op_grid, tensor_op_plan
from tests import byte_movers_ref as R

GROUPS = R.groups()


def _plan(c: R.Case, fn=tensor_op_plan):
    op, rows, row_bytes, isz, tested, kw = R.plan_args(c)
    return fn(op, rows, row_bytes, isz, [R.off(c, n) * isz for n in tested], **kw)


# ---- 1. the plan ----------------------------------------------------------------------------------------------------------------
def test_tensor_op_plan_reports_the_leaf_of_every_case():
    for c in R.CASES:
        if R.plan_args(c) is None:
            assert c.leaf is None and c.fam in ("seq_copy", "position_ids", "check_eos", "cumsum", "batch_inputs"), c
        else:
            assert _plan(c) == c.leaf, c


def test_the_table_reaches_every_leaf_of_every_op():
    printed: dict = {}
    for op in TENSOR_PLAN_OPS:
        for rows, row_bytes, isz in ((3, 96, 2), (3, 88, 2), (3, 92, 2), (3, 90, 2), (3, 45, 1), (3, 128, 2), (2, 16384 * 4, 4), (2, 16383 * 2, 2), (2, 64, 8)):
            for bits in range(16):
                q = min(row_bytes & -row_bytes, 16)                             # the widest power of two that divides the row
                kw = {"widths": (row_bytes - 2 * q, q, q)} if op == "split_qkv" else {}
                try:
                    printed.setdefault(op, set()).add(tensor_op_plan(op, rows, row_bytes, isz, [bits], **kw))
                except ValueError:
                    pass
    five = set(R.VEC_LEAVES)
    assert printed == {"transpose_2d": {"tile64"}, "transpose_batched": {"tile64"}, "transpose_3d_021": five, "repeat_interleave": five,
                       "split_qkv": five, "embedding_lookup": five, "slice_rows": five, "kv_cache_write": five, "scatter_last_logits": five,
                       "paged_cache_write": {"vec16"}, "argmax": {"block256", "block1024"}}
    reached: dict = {}
    for c in R.CASES:
        if R.plan_args(c):
            reached.setdefault(R.plan_args(c)[0], set()).add(c.leaf)
    assert reached == printed
    # both modes of the row map, and every entry point that reaches a width-picking kernel, on all five widths
    for entry in ("transpose_3d_021", "transpose_102", "transpose_4d_0213", "repeat_interleave_axis1", "embedding_lookup", "embedding_lookup_ptr",
                  "embedding_lookup_batch", "gather_embeddings", "slice_rows_range_ptr", "kv_cache_update_gqa", "kv_cache_update_gqa_ptr",
                  "kv_cache_prefill_gqa", "split_qkv_batch", "scatter_last_token_logits"):
        assert {c.leaf for c in R.CASES if c.entry == entry} == five, entry
    # split_qkv never goes below one element
    assert {c.leaf for c in R.CASES if c.fam == "split_qkv" and c.item == "f32"} == {"vec4", "vec8"}
    assert tensor_op_plan("split_qkv", 7, 20, 4, [4], widths=(12, 4, 4)) == "vec4" and tensor_op_plan("split_qkv", 7, 20, 2, [2], widths=(10, 6, 4)) == "vec2"
    # argmax: both block sizes in every dtype, n on both sides of the switch
    for item in ("f32", "f16", "bf16"):
        assert {(c.shape[1], c.leaf) for c in R.CASES if c.fam == "argmax" and c.item == item} >= \
            {(n, "block1024" if n >= 16384 else "block256") for n in R.ARGMAX_N}


SUPPLIED = {"transpose": ("in",), "T": ("in",), "transpose_3d_012": ("in", "out"), "transpose_4d_0132": ("in", "out"), "transpose_3d_021": ("in", "out"),
            "transpose_102": ("in",), "transpose_4d_0213": ("in", "out"), "repeat_interleave_axis1": ("in",), "split_qkv_batch": ("qkv", "q", "k", "v"),
            "embedding_lookup": ("table", "out"), "embedding_lookup_ptr": ("table", "out"), "embedding_lookup_batch": ("table", "out"),
            "gather_embeddings": ("table",), "slice_rows_range_ptr": ("table", "out"), "kv_cache_update_gqa": ("cache",),
            "kv_cache_update_gqa_ptr": ("new_kv", "cache"), "kv_cache_prefill_gqa": ("new_kv",), "kv_cache_update": ("new_kv", "cache"),
            "kv_cache_prefill": ("new_kv", "cache"), "concat_axis0": ("a", "b"), "reshape_copy": ("in", "out"), "reshape": ("in",),
            "argmax_rows_out": ("x", "out"), "scatter_last_token_logits": ("logits", "out"), "copy_to_paged_cache": ("k", "v", "k_cache", "v_cache")}


def test_every_operand_a_caller_supplies_is_misaligned_in_some_case():
    """Per entry point, the operands listed in SUPPLIED sit off the allocation's alignment in at least one case, and across the
    entry points of one launcher every operand the launcher tests does.  The int32 index buffers stay aligned; the paged-cache
    write has one width and tests no address, so its views move by 16 bytes and stay on a 16-byte boundary."""
    for entry, names in SUPPLIED.items():
        off = {n for c in R.CASES if c.entry == entry for n, _ in c.mis}
        assert off == set(names), (entry, off)
    by_launcher: dict = {}
    for c in R.CASES:
        if R.plan_args(c) and R.plan_args(c)[4]:
            by_launcher.setdefault(R.plan_args(c)[0], set()).update(n for n, _ in c.mis)
    assert by_launcher == {"transpose_3d_021": {"in", "out"}, "repeat_interleave": {"in"}, "split_qkv": {"qkv", "q", "k", "v"},
                           "embedding_lookup": {"table", "out"}, "slice_rows": {"table", "out"}, "kv_cache_write": {"new_kv", "cache"},
                           "scatter_last_logits": {"logits", "out"}}           # repeat_interleave_axis1 allocates its own output
    for c in R.CASES:
        for n, k in c.mis:
            byte = k * R.ITEM[R.operands(c)[n].item]
            assert (byte % 16 == 0) == (c.fam == "paged_write") and k > 0, c
    # the offsets 1, 2 and 4 elements into an allocation, on every kernel that picks a width
    for fam in ("row_map", "gather", "slice", "kv_write", "scatter_last"):
        assert {k for c in R.CASES if c.fam == fam for _, k in c.mis} == {1, 2, 4}, fam


def test_every_wrap_case_wraps_its_grid_with_no_row_to_spare():
    wraps = [c for c in R.CASES if c.wrap]
    for c in wraps:
        items, grid = R.wrap_items(c), _plan(c, tensor_op_grid)
        assert grid == R.CAP and items > grid * R.BLOCK, (str(c), items, grid)
        op, rows, row_bytes, isz, _, kw = R.plan_args(c)
        per_row = items // rows
        assert per_row * rows == items and (rows - 1) * per_row <= grid * R.BLOCK, str(c)       # one row fewer would not wrap
    assert {(c.entry, c.leaf) for c in wraps} == {("transpose_3d_021", "vec2"), ("transpose_3d_021", "vec16"), ("repeat_interleave_axis1", "vec2"),
                                                   ("split_qkv_batch", "vec2"), ("slice_rows_range_ptr", "vec2"), ("kv_cache_prefill_gqa", "vec2"),
                                                   ("reshape_and_cache", "vec16")}
    # the 16-byte wrap is exactly one vector over, and nothing else wraps
    assert R.wrap_items(next(c for c in wraps if (c.entry, c.leaf) == ("transpose_3d_021", "vec16"))) == R.CAP * R.BLOCK + 1
    assert R.wrap_items(next(c for c in wraps if c.fam == "paged_write")) == R.CAP * R.BLOCK + 16
    for c in R.CASES:
        if not c.wrap and c.fam in ("row_map", "split_qkv", "slice", "kv_write", "paged_write"):
            assert _plan(c, tensor_op_grid) * R.BLOCK >= R.wrap_items(c) // R.launches(c), c


def test_grids():
    assert tensor_op_grid("transpose_2d", 129, 200 * 2, 2) == 3 * 4 and tensor_op_grid("transpose_batched", 65, 63, 1, batch=3) == 2 * 1 * 3
    assert tensor_op_grid("embedding_lookup", 5, 90, 2) == 5 and tensor_op_grid("scatter_last_logits", 3, 50257 * 2, 2) == 3
    assert tensor_op_grid("argmax", 3, 151936 * 4, 4) == 3
    assert tensor_op_grid("slice_rows", 4, 96, 2) == 1 and tensor_op_grid("slice_rows", 4, 96, 2, [2]) == 1 and tensor_op_grid("slice_rows", 40, 96, 2, [2]) == 8
    assert tensor_op_grid("kv_cache_write", 1 << 20, 256, 2) == 4096 and tensor_op_grid("paged_cache_write", 18, 256, 2) == 2
    assert tensor_op_grid("split_qkv", 7, 22, 2, widths=(10, 6, 6)) == 1


@pytest.mark.parametrize("args,kw", [(("matmul", 4, 8, 2), {}), (("slice_rows", 0, 8, 2), {}), (("slice_rows", 4, 0, 2), {}), (("slice_rows", 4, 9, 2), {}),
                                     (("transpose_2d", 4, 12, 3), {}), (("transpose_2d", 4, 8, 2), {"batch": 2}), (("transpose_batched", 1, 1, 1), {"batch": 65536}),
                                     (("paged_cache_write", 4, 90, 2), {}), (("argmax", 4, 8, 1), {}), (("argmax", 4, 64, 8), {}),
                                     (("kv_cache_write", 1 << 31, 8, 2), {}), (("transpose_batched", 4, 8, 2), {"batch": 0})], ids=str)
def test_plan_rejects_what_the_entry_points_reject(args, kw):
    with pytest.raises(ValueError, match="pgk_tensor_op_plan"):
        tensor_op_plan(*args, **kw)
    with pytest.raises(ValueError, match="pgk_tensor_op_grid"):
        tensor_op_grid(*args, **kw)


def test_split_qkv_widths_are_required_and_checked():
    for kw in ({}, {"widths": (8, 8)}, {"widths": (8, 8, 4)}):
        with pytest.raises(ValueError, match="widths"):
            tensor_op_plan("split_qkv", 4, 24, 2, **kw)
    with pytest.raises(ValueError, match="widths"):
        tensor_op_plan("slice_rows", 4, 24, 2, widths=(8, 8, 8))


def test_names_and_c_abi():
    assert ops.tensor_op_plan is tensor_op_plan and ops.tensor_op_grid is tensor_op_grid
    assert {"tensor_op_plan", "tensor_op_grid", "TENSOR_PLAN_OPS"} <= set(ops.__all__) and len(set(ops.__all__)) == len(ops.__all__)
    for name, restype in (("pgk_tensor_op_plan", C.c_char_p), ("pgk_tensor_op_grid", C.c_int)):
        argtypes, got = _hip._NON_STATUS[name]
        assert got is restype and list(argtypes) == [C.c_char_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_uint]
        assert name in _hip.EXPORTED_SYMBOLS and hasattr(_hip.load(), name)
    assert not [n for n in _hip.EXPORTED_SYMBOLS if not hasattr(_hip.load(), n)]
    assert _hip.load().pgk_tensor_op_plan(None, 1, 1, 1, 1, 0) is None and _hip.load().pgk_tensor_op_grid(None, 1, 1, 1, 1, 0) == -1
    assert tensor_op_plan("slice_rows", 4, 96, 2, [0x7f00, 0x7f10]) == "vec16" and tensor_op_plan("slice_rows", 4, 96, 2, [0x7f00, 0x7f18]) == "vec8"


# ---- 2. the table covers what the issue names -------------------------------------------------------------------------------------
def test_the_table_covers_every_entry_point_and_edge():
    entries = {c.entry for c in R.CASES}
    assert entries == set(SUPPLIED) | {"argmax", "argmax_int", "argmax_rows", "sample_greedy", "argmax_sample", "reshape_and_cache",
                                       "prepare_position_ids", "check_eos", "compute_cumsum", "prepare_batch_inputs"}
    t = [c for c in R.CASES if c.fam == "transpose"]
    assert {c.item for c in t} == {"u8", "bf16", "f32", "i64"}
    for item in ("u8", "bf16", "f32", "i64"):
        assert {c.shape for c in t if c.item == item and len(c.shape) == 2} == set(R.TRANSPOSE_SHAPES)
        assert {c.shape[0] for c in t if c.item == item and c.entry == "transpose_3d_012"} == {1, 3}
    assert {c.extra[0] for c in R.CASES if c.entry == "repeat_interleave_axis1" and not c.wrap} == {1, 2, 5}
    g = [c for c in R.CASES if c.fam == "gather"]
    assert {c.shape[1] for c in g if c.item == "bf16"} >= {64, 4096} and all(0 in c.extra or 6 in c.extra for c in g)
    assert any(len(set(c.extra)) < len(c.extra) for c in g)                                    # repeated ids
    kv = [c for c in R.CASES if c.fam == "kv_write"]
    assert {c.extra[0] // c.shape[1] for c in kv} >= {1, 2, 4, 5} and any(c.extra[0] != c.extra[1] for c in kv)      # un-expanded caches too
    assert {c.extra[3] for c in kv if c.entry == "kv_cache_update_gqa"} == {0, 9} and all(c.extra[2] == 10 for c in kv if not c.wrap)
    assert {c.extra[3] for c in kv if c.entry == "kv_cache_update_gqa_ptr" and not c.mis} == {9, 10, 12}
    a = [c for c in R.CASES if c.fam == "argmax"]
    for item in ("f32", "f16", "bf16"):
        for n in R.ARGMAX_N:
            kinds = {k for c in a if c.item == item and c.shape[1] == n for k in c.extra}
            assert kinds == {k for k in R.ARGMAX_KINDS if R.argmax_places(k, n) is not None}, (item, n)
        assert {c.shape[0] for c in a if c.item == item} == {1, 3}
    for k, n in (("tie_stride", 16383), ("tie_stride", 16384)):
        i, j = R.argmax_places(k, n)
        assert j - i == R.argmax_block(n) and i % 64 == j % 64                                  # the same thread, two strides
    i, j = R.argmax_places("tie_lanes", 257)
    assert i // 64 == j // 64 and i != j
    i, j = R.argmax_places("tie_waves", 257)
    assert i // 64 != j // 64 and j < 256
    p = [c for c in R.CASES if c.fam == "paged_write" and not c.wrap and not c.mis]
    assert {(c.item, c.shape[2], c.extra[1]) for c in p} == {(i, d, b) for i in ("bf16", "f16") for d in (64, 128) for b in (1, 4, 16)}
    for c in R.CASES:
        if c.fam == "paged_write":
            slots = R.operands(c)["slots"].words
            live = slots[slots >= 0]
            assert len(set(live.tolist())) == live.size and (slots < 0).sum() == 2 and live.min() == 0 and live.max() == c.extra[0] * c.extra[1] - 1
            assert slots[-1] >= 0 and (np.diff(live) < 0).any()                                  # scattered, and the last token is written
    s = [c for c in R.CASES if c.fam == "scatter_last"]
    assert {(c.item, c.shape[1]) for c in s} >= {("f16", 50257), ("f32", 50257), ("f16", 1000)} and {c.item for c in s} >= {"f16", "bf16", "f32"}
    assert any(c.shape[1] * R.ITEM[c.item] < 4096 for c in s) and any(c.shape[1] * R.ITEM[c.item] > 4096 for c in s)
    assert any(1 in c.extra for c in s) and any(max(c.extra) > 1 for c in s)
    assert {n for c in R.CASES if c.fam == "position_ids" for n in c.extra[0]} >= {0, 1, 256, 257}
    assert {(c.shape[0], c.extra[0]) for c in R.CASES if c.fam == "check_eos"} == {(n, h) for n in (1, 256, 257) for h in ("none", "once", "all")}
    assert {c.shape[0] for c in R.CASES if c.fam == "cumsum"} == {1, 2, 1000}
    assert all((R.operands(c)["in"].words == 0).any() for c in R.CASES if c.fam == "cumsum" and c.shape[0] > 2)


def test_ids_slots_and_rows_stay_in_range():
    """A correct kernel never leaves its buffers; where the kernel itself skips a write, the guard holds what an unguarded one would hit."""
    for c in R.CASES:
        o = R.operands(c)
        if c.fam == "gather" and "ids" in o:
            assert o["ids"].words.min() >= 0 and o["ids"].words.max() < c.shape[0]
        if c.fam == "slice":
            assert 0 <= c.extra[0] and c.extra[0] + c.extra[1] <= c.shape[0]
        if c.fam == "scatter_last":
            assert (o["lens"].words >= 1).all() and (o["start"].words + o["lens"].words <= o["logits"].words.shape[0]).all()
        if c.fam == "kv_write":
            hc, _, max_seq, pos = c.extra
            assert pos >= 0 and (pos + c.shape[0] <= max_seq or c.entry.endswith("_ptr"))
            assert (pos + c.shape[0] - max_seq) * c.shape[2] <= o["cache"].guard                 # the row past the last head's end
        if c.fam == "paged_write":
            assert o["k_cache"].guard >= c.shape[1] * c.extra[1] * c.shape[2] and o["slots"].words.min() == -1
        if c.fam == "position_ids":
            assert (o["start"].words + o["lens"].words <= o["out"].words.size).all()


# ---- 3. the planted errors ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(GROUPS), ids=str)
def test_every_applicable_planted_error_changes_a_word(key):
    for c in GROUPS[key]:
        o = R.operands(c)
        exp = R.expected(c, o)
        assert set(exp) == set(R.outputs(c, o))
        for n, e in exp.items():
            assert e.shape == o[n].words.shape and e.dtype == o[n].words.dtype, (str(c), n)
        for name in R.applicable(c, o):
            bad = R.mutate(c, name, o, exp)
            assert any((bad[n] != exp[n]).any() for n in exp), f"{c}: planted error {name} leaves the output as it is"


def test_planted_errors_cover_the_list():
    seen: dict = {}
    for c in R.CASES:
        for m in R.applicable(c, R.operands(c)):
            seen.setdefault(m, set()).add(c.fam)
    assert set(seen) == set(R.PLANTED)
    assert seen["swap_in_ragged_tile"] == {"transpose"} and seen["tile_for_repeat"] == {"row_map"} and seen["head_mod_for_div"] == {"kv_write"}
    assert seen["position_plus_one"] == {"kv_write", "seq_copy"} and seen["k_v_exchanged"] == seen["slot_div_mod_exchanged"] == {"paged_write"}
    assert seen["start_plus_len"] == {"scatter_last"} and seen["inclusive_sum"] == {"cumsum"}
    assert seen["highest_index_on_ties"] == seen["first_wave_only"] == seen["nan_wins"] == {"argmax"}
    assert seen["drop_second_trip"] == {"row_map", "split_qkv", "slice", "kv_write", "paged_write"}
    movers = {"row_map", "split_qkv", "gather", "slice", "kv_write", "paged_write", "scatter_last", "seq_copy"}
    assert seen["wrong_width_stride"] == movers and seen["drop_last_vector"] == movers | {"check_eos"}
    assert seen["row_off_by_one"] == movers | {"transpose", "position_ids", "check_eos", "cumsum"}
    # per item type and block size of argmax
    for item in ("f32", "f16", "bf16"):
        for leaf in ("block256", "block1024"):
            got = {m for c in R.CASES if (c.fam, c.item, c.leaf) == ("argmax", item, leaf) for m in R.applicable(c, R.operands(c))}
            assert got == {"highest_index_on_ties", "first_wave_only", "nan_wins"}, (item, leaf)


def test_inputs_never_hold_the_canary():
    for c in R.CASES:
        if c.wrap or c.fam == "argmax":
            continue
        for n, o in R.operands(c).items():
            if o.role in ("in", "inout") and o.item != "i32":
                assert not (o.words == R.WORD[o.item](R.CANARY[o.item])).any(), (str(c), n)


def test_argmax_rule_is_not_numpys():
    nan, inf = np.nan, np.inf
    assert R.argmax_rule([1, nan, 3, 3]) == 2 and int(np.argmax([1, nan, 3, 3])) == 1          # NaN never wins
    assert R.argmax_rule([nan, nan]) == 0 and R.argmax_rule([-inf, -inf]) == 0 and R.argmax_rule([nan, -inf, nan]) == 0
    assert R.argmax_rule([-1, -0.0, 0.0]) == 1 and R.argmax_rule([-1, 0.0, -0.0]) == 1 and R.argmax_rule([inf, 2, inf]) == 0
    assert R.argmax_rule([-inf, -5]) == 1 and R.argmax_rule([7]) == 0
