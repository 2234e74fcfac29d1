"""CPU side of the exact GEMM checks (tests/gemm_exact_ref.py, tests/test_gemm_exact_gpu.py): for every case of the table

  * the float64 product is exactly representable in the output type, so the GPU file may compare words;
  * every planted error (a dropped 8-wide K chunk, a dropped K tail, rows shifted by one, two swapped columns, no bias on the
    last column, a neighbouring scale block, a transposed tile) changes at least one output word, so the GPU file would notice;
  * gemm_plan, the host-side query built from the decision functions the dispatchers switch on, reports the leaf the table
    names - and the table reaches every leaf gemm_plan can print, or lists it as unreachable with the argument.

Nothing here needs a device: the plan is decided on the host.
"""

from __future__ import annotations

import ctypes as C
import sys

import numpy as np
import pytest

from pygpukit_amd import _hip
from pygpukit_amd.ops.matmul import gemm_plan
from tests import gemm_exact_ref as R

MM = sys.modules["pygpukit_amd.ops.matmul"]      # the attribute ops.matmul is the matmul function
ENV = ("PGK_GEMM256", "PGK_GEMM256S")


def _setenv(monkeypatch, env=()):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for name, value in env:
        monkeypatch.setenv(name, value)


def _plan(monkeypatch, c: R.Case) -> str:
    _setenv(monkeypatch, c.env)
    return gemm_plan(c.op, c.m, c.n, c.k, R.DTYPE_NAME[c.dtype], c.aligned)


# ---- 1. representability --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=str)
def test_expected_output_is_exactly_representable(case):
    o = R.make(case)
    e = o.expected
    np.testing.assert_array_equal(R.round_to(e, case.dtype), e)
    unit = 1.0
    if o.sw is not None:
        unit = min(R.SCALE_W) * (min(R.SCALE_A) if o.sa is not None else 1.0)
        if case.dtype == "bf16":
            assert np.abs(e).max() <= 256 * unit                      # bf16: 8 significant bits of the smallest scale product
    np.testing.assert_array_equal(e / unit, np.rint(e / unit))        # whole multiples of it
    # every partial sum is bounded by the sum of the magnitudes: below 2**24 units, fp32 adds them exactly in any order
    sw = None if o.sw is None else np.abs(o.sw)
    bound = R.product(np.abs(o.a), np.abs(o.w), None if o.bias is None else np.abs(o.bias), o.sa, sw)
    assert bound.max() / unit < 2 ** 24
    assert np.abs(e).max() > 0 and len(np.unique(e)) > 4


def test_operands_are_what_the_module_says():
    for case in (R.CASES[0], next(c for c in R.CASES if c.leaf == "fp8_128"), next(c for c in R.CASES if c.leaf == "wsgemm_mt8_fp8")):
        o = R.make(case)
        if o.sw is None:
            assert set(np.unique(o.a)) <= {-1.0, 0.0, 1.0} and set(np.unique(o.w)) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
            assert o.bias[-1] != 0 and np.abs(o.bias).max() <= 4
            continue
        assert np.abs(o.w).max() <= 4 and np.abs(o.a).max() <= 2 and (o.sa is None or np.abs(o.w).max() <= 2)
        assert (o.sw[:, 1:] != o.sw[:, :-1]).all() and (o.sw[1:] != o.sw[:-1]).all()
        if o.sa is not None:
            assert (o.sa[:, 1:] != o.sa[:, :-1]).all() and (o.sa[1:] != o.sa[:-1]).all()
    table = R.O.fp8_e4m3_table()
    x = np.arange(-4, 5)
    np.testing.assert_array_equal(table[R.fp8_encode(x)], x.astype(np.float32))


# ---- 2. every planted error is visible ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=str)
def test_every_mutant_changes_at_least_one_output_word(case):
    want = R.expected_words(case)
    muts = R.mutants(case)
    need = {"drop_k_chunk", "drop_k_tail", "swap_columns"}
    if case.m > 1:
        need |= {"shift_rows", "transpose_tile"}
    if case.bias:
        need.add("no_bias_on_last_column")
    if case.op in R.FP8_OPS:                                             # every fp8 case has at least two 128-k blocks
        assert case.k >= 256
        need.add("neighbour_w_scale_block")
        if case.n > 128:
            need.add("neighbour_w_scale_row_block")
    if case.op == "fp8_nt":
        need.add("neighbour_a_scale_block")
    assert need <= set(muts), need - set(muts)
    for name, out in muts.items():
        changed = int((R.to_words(out, case.dtype) != want).sum())
        assert changed > 0, f"{case}: mutant {name} returns the expected words"


def test_the_old_bars_do_not_see_one_wrong_word():
    """The contrast: one wrong element, or a whole wrong row at M = 2048, passes the whole-tensor bars the op tests use."""
    from tests.conftest import rel_err

    case = next(c for c in R.CASES if c.leaf == "mfma_128x128_B_NT")
    e = R.make(case).expected
    one = e.copy()
    one[-1, -1] += 64.0
    row = e.copy()
    row[7] = np.roll(e, 1, axis=0)[7]
    assert rel_err(one, e) < 1e-2 and rel_err(row, e) < 5e-2
    assert (R.to_words(one, "bf16") != R.to_words(e, "bf16")).sum() == 1


# ---- 3. the plan: the table's leaves, and every leaf ---------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=str)
def test_gemm_plan_reports_the_leaf_of_the_case(case, monkeypatch):
    assert _plan(monkeypatch, case) == case.leaf


def test_every_leaf_is_reached_or_listed_as_unreachable():
    reached = {R.family(c.leaf) for c in R.CASES}
    assert not reached & R.UNREACHABLE
    assert reached | R.UNREACHABLE == R.all_leaves(), (R.all_leaves() - reached - R.UNREACHABLE, reached - R.all_leaves())
    # and for every dtype that can reach it: the 16-bit MFMA tiles in bf16 and f16, the GEMV and fallback kernels in all three
    by_dtype = {(R.family(c.leaf), c.dtype) for c in R.CASES}
    for leaf in reached:
        if leaf.endswith("_B_NN") or leaf == "simple_nn":
            want = ("bf16", "f16") if leaf != "simple_nn" else ("bf16", "f16", "f32")
        elif leaf.startswith("gemv_fast") or leaf in ("gemv_generic", "simple_nt"):
            want = ("bf16", "f16", "f32")
        elif leaf.endswith("_B_NT"):
            want = ("f16", "bf16") if leaf in ("mfma_128x32_B_NT", "mfma_64x64_B_NT", "mfma_128x128_B_NT") else ("f16",)
        else:
            want = ("bf16",)
        for dt in want:
            assert (leaf, dt) in by_dtype, (leaf, dt)


def test_unreachable_leaves_are_unreachable(monkeypatch):
    """Sweeps the tile choice over M and N on the host: no shape prints a leaf of UNREACHABLE, through any entry point."""
    seen = set()
    ms = [1, 8, 9, 16, 32, 33, 64, 65, 128, 129, 256, 300, 1000, 2048, 4096, 8192, 16384, 40000]
    ns = [128, 256, 1024, 2048, 4096, 8192, 16384, 32768, 65536, 131072]
    for force in (None, "0", "1"):
        _setenv(monkeypatch, () if force is None else (("PGK_GEMM256", force),))
        for m in ms:
            for n in ns:
                seen |= {gemm_plan("nt", m, n, 72, "bfloat16"), gemm_plan("nt", m, n, 72, "float16"), gemm_plan("nn", m, n, 72, "float16"),
                         gemm_plan("nn", m, n, 72, "bfloat16"), gemm_plan("w8a16_nk", m, n, 128, "bfloat16"),
                         gemm_plan("w8a16_kn", m, n, 128, "bfloat16"), gemm_plan("nt", m, n + 8, 64, "bfloat16")}
    assert not seen & R.UNREACHABLE, seen & R.UNREACHABLE
    assert {R.family(s) for s in seen} <= R.all_leaves(), seen - R.all_leaves()


def test_plan_follows_the_environment_per_call(monkeypatch):
    _setenv(monkeypatch)
    assert gemm_plan("nt", 300, 520, 192, "bfloat16") == "gemm128s"
    assert gemm_plan("fp8_nt", 512, 512, 256, "bfloat16") == "fp8_128"
    assert gemm_plan("nt", 4096, 12288, 4096, "bfloat16") == "gemm256s"            # 16 x 48 = 768 tiles >= 192: on by itself
    assert gemm_plan("fp8_nt", 4096, 12288, 4096, "bfloat16") == "fp8_256"
    monkeypatch.setenv("PGK_GEMM256", "1")
    assert gemm_plan("nt", 300, 520, 192, "bfloat16") == "gemm256s" and gemm_plan("nt", 300, 576, 192, "bfloat16") == "gemm256s_n192"
    assert gemm_plan("nt", 300, 520, 72, "bfloat16") == "mfma_128x32_B_NT"          # K % 64 != 0: neither staged kernel
    assert gemm_plan("nt", 300, 520, 192, "float16") == "mfma_128x32_B_NT"          # the staged kernels are bf16
    assert gemm_plan("fp8_nt", 512, 512, 256, "bfloat16") == "fp8_256" and gemm_plan("fp8_nt", 300, 520, 384, "bfloat16") == "fp8_128"
    monkeypatch.setenv("PGK_GEMM256S", "0")
    assert gemm_plan("nt", 300, 576, 192, "bfloat16") == "gemm256_lockstep"
    assert gemm_plan("w8a16_nk", 300, 256, 256, "bfloat16") == "dequant+gemm256_lockstep"
    monkeypatch.setenv("PGK_GEMM256", "0")
    assert gemm_plan("nt", 4096, 12288, 4096, "bfloat16") == "gemm128s"
    assert gemm_plan("w8a16_nk", 300, 256, 256, "bfloat16") == "mfma_128x32_B_NT_FP8"


def test_plan_alignment_and_thresholds(monkeypatch):
    _setenv(monkeypatch)
    assert gemm_plan("nt", 4, 64, 128, "bfloat16", aligned=False) == "gemv_generic"
    assert gemm_plan("nt", 64, 64, 128, "bfloat16", aligned=False) == "simple_nt"
    assert gemm_plan("nn", 64, 64, 128, "float16", aligned=False) == "simple_nn"
    assert gemm_plan("nt", 1, 64, 32768, "bfloat16") == "gemv_fast_m1" and gemm_plan("nt", 1, 64, 32776, "bfloat16") == "wsgemm_mt1"
    assert gemm_plan("nt", 8, 64, 4096, "float16") == "gemv_fast_m8" and gemm_plan("nt", 8, 64, 4104, "float16") == "mfma_32x32_B_NT"
    assert gemm_plan("nt", 8, 64, 2048, "float32") == "gemv_fast_m8" and gemm_plan("nt", 8, 64, 2052, "float32") == "gemv_generic"
    assert gemm_plan("nt", 128, 64, 64, "bfloat16") == "wsgemm_mt8" and gemm_plan("nt", 129, 64, 64, "bfloat16") == "gemm128s"
    assert gemm_plan("nt", 129, 60, 64, "bfloat16") == "mfma_128x32_B_NT"           # N % 8 != 0 keeps it off the staged kernel
    assert gemm_plan("gemv_fp8", 16, 128, 128, "bfloat16") == "gemv_fp8_m8x2"


@pytest.mark.parametrize("args", [("tn", 4, 128, 128, "bfloat16"), ("nt", 0, 128, 128, "bfloat16"), ("nt", 4, 128, 128, "int32"),
                                  ("fp8_nt", 4, 128, 100, "bfloat16"), ("w8a16_nk", 4, 100, 128, "bfloat16"), ("w8a16_kn", 4, 128, 128, "float16"),
                                  ("gemv_fp8", 8, 128, 4224, "bfloat16")], ids=str)
def test_plan_rejects_what_the_entry_points_reject(args):
    with pytest.raises(ValueError, match="pgk_gemm_plan"):
        gemm_plan(*args)
    with pytest.raises(ValueError):
        gemm_plan("w8a16_nk", 4, 128, 128, "bfloat16", aligned=False)


def test_names_and_c_abi():
    assert MM.gemm_plan is gemm_plan and "gemm_plan" in MM.__all__ and len(set(MM.__all__)) == len(MM.__all__)
    assert MM.GEMM_PLAN_OPS == ("nt", "nn", "w8a16_nk", "w8a16_kn", "gemv_fp8", "fp8_nt") and {c.op for c in R.CASES} == set(MM.GEMM_PLAN_OPS)
    argtypes, restype = _hip._NON_STATUS["pgk_gemm_plan"]
    assert restype is C.c_char_p and list(argtypes) == [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    assert "pgk_gemm_plan" in _hip.EXPORTED_SYMBOLS and hasattr(_hip.load(), "pgk_gemm_plan")
    assert _hip.load().pgk_gemm_plan(None, 1, 1, 1, 0, 1) is None


def test_failure_message_names_the_place_and_the_usual_wrong_answers():
    """What the GPU file prints on a mismatch, run here on planted errors: (m, n), tile coordinates, and what came back instead."""
    case = next(c for c in R.CASES if c.leaf == "gemm128s" and c.m == 300)
    want = R.expected_words(case)
    muts = R.mutants(case)
    for name, phrase in (("no_bias_on_last_column", "the sum without the bias"), ("shift_rows", "the row above"),
                         ("drop_k_tail", "the sum without the last K tile")):
        msg = R.explain(case, R.to_words(muts[name], case.dtype), want)
        assert phrase in msg and "tile (" in msg and "128 x 128 x 64" in msg, msg
    msg = R.explain(case, R.to_words(muts["no_bias_on_last_column"], case.dtype), want)
    assert "(0, 519) tile (0, 4) at (0, 7): expected " in msg and "columns [519] (1)" in msg and "300 of 156000 words differ" in msg, msg
    assert len(R.explain(case, R.to_words(muts["shift_rows"], case.dtype), want).splitlines()) == 14      # header, a dozen, summary
