"""CPU side of the per-element base op checks (tests/base_ops_ref.py, tests/test_base_ops_gpu.py): for every case of the table

  * base_op_plan, the host-side query built from the functions the launchers call (csrc/base_plan.h), reports the leaf the
    table names, the table reaches every leaf it can print, and every wrap case really wraps its grid (base_op_grid);
  * where a case is compared under a bar, two float32 NumPy emulations - sums left to right and sums as a binary tree - stay
    inside it on every element, so the bar does not reject a correct float32 implementation;
  * every applicable planted error (a dropped tail, elements shifted by one, the neighbouring column's gamma or bias, the
    previous row's statistic, no eps, variance without mean subtraction, no residual, RoPE with the sign of sin flipped / pairs
    (d, d + 1) / the table row of s + 1 / k heads found with q's head count, softmax without max subtraction, mean over n - 1,
    max without the last element, a truncating cast) moves at least one element outside its bar or changes a word, so the GPU
    file would notice;
  * where a case is compared as words, the expected value is representable and the integer sums stay below 2^24.

Nothing here needs a device: the plan is decided on the host.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from pygpukit_amd import _hip, ops
from pygpukit_amd.ops.plan import BASE_PLAN_OPS, base_op_grid, base_op_plan
from tests import base_ops_ref as R

GROUPS = R.groups()


def _plan(c: R.Case, fn=base_op_plan):
    op, rows, features = R.plan_args(c)
    return fn(op, rows, features, R.DTYPE_NAME[c.dtype], not c.mis)


# ---- 1. the plan ----------------------------------------------------------------------------------------------------------------
def test_base_op_plan_reports_the_leaf_of_every_case():
    for c in R.CASES:
        if R.plan_args(c) is None:
            assert c.leaf is None and c.fam in ("softmax", "sum_axis"), c          # one kernel, one block per row / 256 columns
        else:
            assert _plan(c) == c.leaf, c


def test_the_table_reaches_every_leaf_in_every_dtype():
    printed = set()
    for op in BASE_PLAN_OPS:
        for dt in R.DTYPES:
            for rows, features in ((1, 2), (5, 8), (5, 16), (5, 26), (3, 4104), (3, 2052), (1 << 22, 2)):
                for aligned in (True, False):
                    printed.add(base_op_plan(op, rows, features, R.DTYPE_NAME[dt], aligned))
    assert printed == R.LEAVES
    reached = {(c.leaf, c.dtype) for c in R.CASES if c.leaf}
    assert reached == {(leaf, dt) for leaf in R.LEAVES for dt in R.DTYPES}
    # every op of the query has cases, and each flat / row / norm op reaches both of its leaves
    by_op = {}
    for c in R.CASES:
        if R.plan_args(c):
            by_op.setdefault(R.plan_args(c)[0], set()).add(c.leaf)
    assert set(by_op) == set(BASE_PLAN_OPS)
    for op in ("binary", "activation", "glu"):
        assert by_op[op] == {"ew_vec", "ew_scalar"}
    for op in ("glu_packed", "bias_add"):
        assert by_op[op] == {"row_vec", "row_scalar"}
    for op in R.NORM_MODES:
        assert by_op[op] == {"norm_wave", "norm_block"}


def test_every_misalignable_operand_is_misaligned_in_turn():
    for fam, op in (("binary", "add"), ("binary", "add_inplace"), ("act", "exp"), ("glu", "geglu"), ("glu_packed", "silu"), ("bias_add", "add"),
                    ("norm", "rmsnorm"), ("norm", "rmsnorm_residual"), ("norm", "layernorm")):
        for dt in R.DTYPES:
            cases = [c for c in R.CASES if (c.fam, c.op, c.dtype) == (fam, op, dt)]
            off = {m for c in cases for m in c.mis}
            assert off == set(R.operands(cases[0])), (fam, op, dt, off)
            for c in cases:
                if c.mis and fam == "norm":
                    assert c.shape[1] % R.NVEC[dt] == 0 and c.leaf == "norm_block"      # vector-eligible, kept off by the pointer alone


def test_every_wrap_case_wraps_its_grid():
    wraps = [c for c in R.CASES if c.wrap]
    for c in wraps:
        items, per_block = R.wrap_work(c)
        grid = _plan(c, base_op_grid)
        cap = R.RD_CAP if c.fam in ("clamp", "where", "reduce") else R.EW_CAP
        assert grid == cap and grid * per_block < items, (str(c), grid, per_block, items)
        N = R.NVEC[c.dtype]
        if c.leaf == "ew_vec":                      # exactly one whole vector and a 3-element tail are left for the second trip
            assert c.n == cap * R.BLOCK * N + N + 3 and c.n // N == grid * R.BLOCK + 1
        elif c.leaf == "ew_scalar":
            assert c.n == cap * R.BLOCK + 5
        elif c.fam in ("clamp", "where"):
            assert c.n == cap * R.BLOCK + 1         # the smallest n above grid * 256
        elif c.leaf in ("row_vec", "row_scalar"):
            rows, f = c.shape
            smaller = (rows - 1) * f // (N if c.leaf == "row_vec" else 1)
            assert smaller <= cap * R.BLOCK         # one row fewer would not wrap
    # one per kernel template and dtype
    want = {(fam, leaf, dt) for dt in R.DTYPES for fam, leaves in (("binary", ("ew_vec", "ew_scalar")), ("act", ("ew_vec", "ew_scalar")),
            ("glu", ("ew_vec", "ew_scalar")), ("glu_packed", ("row_vec", "row_scalar")), ("bias_add", ("row_vec", "row_scalar")),
            ("clamp", ("ew_stride",)), ("where", ("ew_stride",)), ("rope", ("rope_pairs",)), ("cast", ("cast_x4",)),
            ("reduce", ("reduce_tree",))) for leaf in leaves}
    assert {(c.fam, c.leaf, c.dtype) for c in wraps} == want
    assert {(c.dtype, c.extra[0]) for c in wraps if c.fam == "cast"} == set(R.CAST_PAIRS)
    assert {(c.dtype, c.extra[0]) for c in wraps if c.fam == "rope"} == {(dt, t) for dt in R.DTYPES for t in ("f32", dt)}
    # below the cap nothing wraps: the grid covers the work
    for c in R.CASES:
        if not c.wrap and R.plan_args(c) and c.fam != "norm":
            items, per_block = R.wrap_work(c)
            assert _plan(c, base_op_grid) * per_block >= items, c


def test_grid_of_the_row_kernels():
    assert base_op_grid("rmsnorm", 5, 256, "float32") == 2 and base_op_grid("rmsnorm", 5, 257, "float32") == 5      # 4 rows per block / a block per row
    assert base_op_grid("layernorm", 5, 256, "bfloat16", aligned=False) == 5
    assert base_op_grid("binary", 3, 1, "float32") == 1 and base_op_grid("binary", 1024, 1, "float32") == 2          # n / N + 1 vectors
    assert base_op_grid("cast", 1 << 30, 1, "float16") == 2048 and base_op_grid("where", 1 << 30, 1, "float16") == 1024
    assert base_op_grid("rope", 12, 128, "bfloat16") == 3 and base_op_grid("bias_add", 3, 24, "float16") == 1


@pytest.mark.parametrize("args", [("matmul", 4, 8, "float32"), ("binary", 0, 1, "float32"), ("binary", 4, 1, "int32"), ("rmsnorm", 4, 0, "float32"),
                                  ("rope", 4, 3, "float16"), ("bias_add", 1 << 32, 8, "float32")], ids=str)
def test_plan_rejects_what_the_entry_points_reject(args):
    with pytest.raises(ValueError, match="pgk_base_op_plan"):
        base_op_plan(*args)
    with pytest.raises(ValueError, match="pgk_base_op_grid"):
        base_op_grid(*args)


def test_names_and_c_abi():
    assert ops.base_op_plan is base_op_plan and ops.base_op_grid is base_op_grid
    assert {"base_op_plan", "base_op_grid"} <= set(ops.__all__) and len(set(ops.__all__)) == len(ops.__all__)
    for name, restype in (("pgk_base_op_plan", C.c_char_p), ("pgk_base_op_grid", C.c_int)):
        argtypes, got = _hip._NON_STATUS[name]
        assert got is restype and list(argtypes) == [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_int]
        assert name in _hip.EXPORTED_SYMBOLS and hasattr(_hip.load(), name)
    assert _hip.load().pgk_base_op_plan(None, 1, 1, 0, 1) is None and _hip.load().pgk_base_op_grid(None, 1, 1, 0, 1) == -1


# ---- 2. the bars admit float32 arithmetic, 3. and no planted error ---------------------------------------------------------------
@pytest.mark.parametrize("key", list(GROUPS), ids=str)
def test_emulations_stay_inside_and_planted_errors_fall_outside(key):
    for c in GROUPS[key]:
        for how in ("seq", "pairwise"):
            got = R.emulate(c, how)
            assert not any(m.any() for m in R.mismatches(c, got).values()), R.explain(c, got)
        muts = R.mutations(c)
        for name in muts:
            bad = R.mismatches(c, R.emulate(c, "f64", name))
            assert any(m.any() for m in bad.values()), f"{c}: planted error {name} stays inside the bars"


def test_planted_errors_cover_the_list():
    seen = {(c.fam, m) for c in R.CASES for m in R.mutations(c)}
    for fam in ("binary", "act", "glu", "glu_packed", "bias_add", "cast", "norm", "clamp", "where"):
        assert (fam, "drop_tail") in seen and (fam, "shift_one") in seen, fam
    assert {m for f, m in seen if f == "norm"} == {"drop_tail", "shift_one", "neighbour_column", "previous_row_statistic", "no_eps",
                                                   "variance_without_mean", "no_residual"}
    assert ("bias_add", "neighbour_column") in seen and ("cast", "truncate") in seen
    assert {m for f, m in seen if f == "rope"} == {"sin_sign", "pairs_adjacent", "table_row_plus_one", "k_heads_as_q_heads"}
    assert {m for f, m in seen if f == "softmax"} == {"drop_last", "no_max_subtraction"}
    assert {m for f, m in seen if f == "reduce"} == {"ignore_last", "mean_n_minus_1"} and ("sum_axis", "drop_last") in seen
    # per mode and dtype of the norms, and the truncating cast on every narrowing pair
    for op in R.NORM_MODES:
        for dt in R.DTYPES:
            got = {m for c in R.CASES if (c.fam, c.op, c.dtype) == ("norm", op, dt) for m in R.mutations(c)}
            assert {"no_eps", "previous_row_statistic", "neighbour_column"} <= got and ("no_residual" in got) == (op == "rmsnorm_residual")
    assert {(c.dtype, c.extra[0]) for c in R.CASES if c.fam == "cast" and "truncate" in R.mutations(c)} == \
        {("f32", "bf16"), ("f32", "f16"), ("bf16", "f16"), ("f16", "bf16")}
    for op in ("max", "min"):                       # the extreme is planted at every index the issue names
        for dt in R.DTYPES:
            at = {c.extra[0] for c in R.CASES if (c.fam, c.op, c.dtype) == ("reduce", op, dt) and c.n == 2 * 1024 * 256 + 7}
            assert at == {0, 255, 256, 1024 * 256, 2 * 1024 * 256 + 6}


def test_measured_use_of_the_bars_in_float32():
    """The record in base_ops_ref.MEASURED: the share of each bar the float32 emulations use.  No bar is derived from it."""
    worst: dict = {}
    for c in R.CASES:
        if c.dtype == "f32" and not R.is_exact(c) and not c.wrap:
            for how in ("seq", "pairwise"):
                worst[R.bar_family(c)] = max(worst.get(R.bar_family(c), 0.0), R.used(c, R.emulate(c, how)))
    print({k: round(v, 3) for k, v in sorted(worst.items())})
    assert set(worst) == set(R.MEASURED)
    for k, v in worst.items():
        assert v < 1.0 and abs(v - R.MEASURED[k]) < 0.02, (k, v, R.MEASURED[k])


# ---- 4. exact cases -------------------------------------------------------------------------------------------------------------
def test_exact_cases_are_representable_and_integer_sums_stay_small():
    for c in R.CASES:
        if not R.is_exact(c) or c.wrap and c.fam not in ("reduce", "rope"):
            continue
        ins = R.inputs(c)
        exp = R.expected(c)
        assert all(e[0] == "words" for e in exp.values()), c
        if c.fam in ("reduce", "sum_axis") and c.op not in ("max", "min"):
            x = np.asarray(ins["x"], np.float64)
            assert (x == np.rint(x)).all() and np.abs(x).sum() < 2 ** 24, c        # any partial sum, in any order, is exact in float32
            total = x.sum() if c.fam == "reduce" else x.sum(axis=1 if c.op == "axis1" else 0)
            np.testing.assert_array_equal(R.rounded(total, c.dtype), np.asarray(total, np.float32), err_msg=str(c))
            if c.op != "mean":
                np.testing.assert_array_equal(R.from_words(exp["out"][1], c.dtype).reshape(-1), np.asarray(total, np.float32).reshape(-1))
            if c.fam == "reduce" or c.op == "axis1":
                assert (x.reshape(-1, x.shape[-1])[:, -1] != 0).all()                # the last element counts
        if c.fam == "rope":                                                          # every product and sum is exact
            for name in ("q", "k"):
                v = R.compute(c, ins, np.float64)[name]
                np.testing.assert_array_equal(R.rounded(v, c.dtype), np.asarray(v, np.float32), err_msg=str(c))
                assert (v * 2 == np.rint(v * 2)).all() and np.abs(v).max(initial=0) <= 16
            half = c.shape[3] // 2
            assert np.isnan(ins["cos"][:, half:]).all() and np.isnan(ins["sin"][:, half:]).all()
        if c.fam == "reduce" and c.op in ("max", "min"):
            x = ins["x"]
            other = np.delete(x, c.extra[0])
            assert (other < x[c.extra[0]]).all() if c.op == "max" else (other > x[c.extra[0]]).all()


def test_cast_table_holds_the_special_values():
    t = R.cast_table()
    assert np.isnan(t).sum() == 1 and np.isposinf(t).any() and np.isneginf(t).any() and (np.signbit(t) & (t == 0)).any()
    f16 = R.from_words(R.to_words(t, "f16"), "f16")
    bf = R.from_words(R.to_words(t, "bf16"), "bf16")
    at = lambda v: int(np.flatnonzero(t == np.float32(v))[0])      # noqa: E731
    assert f16[at(65519.0)] == 65504.0 and np.isposinf(f16[at(65520.0)]) and np.isposinf(f16[at(3.3895314e38)])
    assert np.isposinf(bf[at(3.4028235e38)]) and bf[at(3.3895314e38)] == np.float32(3.3895314e38) and bf[at(65504.0)] == 65536.0
    assert bf[at(1 + 2.0 ** -8)] == 1.0 and bf[at(1 + 3 * 2.0 ** -8)] == 1 + 2.0 ** -6 and bf[at(1 + 2.0 ** -8 + 2.0 ** -20)] == 1 + 2.0 ** -7
    assert f16[at(1 + 2.0 ** -11)] == 1.0 and f16[at(1 + 3 * 2.0 ** -11)] == 1 + 2.0 ** -9
    assert f16[at(2.0 ** -24)] == 2.0 ** -24 and f16[at(2.0 ** -25)] == 0.0 and f16[at(1.5 * 2.0 ** -25)] == 2.0 ** -24      # subnormal results, a tie to 0
    sub = (np.abs(f16) > 0) & (np.abs(f16) < 2.0 ** -14)
    assert sub.sum() >= 8
    for src, dst in R.CAST_PAIRS:                    # the table goes through every pair, at the front and in the tail
        c = next(c for c in R.CASES if c.fam == "cast" and (c.dtype, c.extra[0]) == (src, dst) and c.n == 1027 and not c.mis)
        x = R.inputs(c)["src"]
        np.testing.assert_array_equal(R.canonical(R.to_words(x[:t.size], src), src), R.to_words(t, src))
        np.testing.assert_array_equal(R.canonical(R.to_words(x[-t.size:], src), src), R.to_words(t[::-1], src))


def test_the_old_bar_does_not_see_what_these_tests_see():
    """The contrast: one wrong tail element, or one element normalised with the neighbouring row's statistic, passes the 1e-2 whole-tensor bar."""
    from tests.conftest import rel_err

    c = next(c for c in R.CASES if (c.fam, c.op, c.dtype, c.shape) == ("norm", "rmsnorm", "bf16", (5, 4096)))
    want = R.expected(c)["out"][1]
    got = R.emulate(c, "f64")
    got["out"][4, -1] = R.emulate(c, "f64", "previous_row_statistic")["out"][4, -1]      # the last element, off by a factor of two
    assert rel_err(R.from_words(got["out"], "bf16"), want) < 1e-2 and R.mismatches(c, got)["out"].sum() == 1
    c = next(c for c in R.CASES if (c.fam, c.op, c.dtype, c.shape) == ("binary", "div", "bf16", (2051,)))
    got = R.emulate(c, "seq")
    got["c"][-1] = np.uint16(0)
    assert rel_err(R.from_words(got["c"], "bf16"), R.expected(c)["c"][1]) < 1e-2 and R.mismatches(c, got)["c"].sum() == 1
