"""CPU side of the exact sampling tests (tests/sampling_ref.py has the construction).

  * precondition: for every case the GPU file runs, the closed-form kept set is what oracle.cpu_ref.sample_token_u
    enumerates at every u used, every u is a float32 in [0, 1], the rows are the same numbers in f32 / f16 / bf16, and
    every graded draw is at least 5e-4 of the kept mass from a boundary;
  * sensitivity: a mutable restatement of the sampler equals the oracle on every case, and each of its mutants (one
    token more or less, ties from the top, signed-zero key order, reciprocal temperature, `>` for `>=` in the nucleus
    and in the draw, nucleus against the whole row, z-descending draw, unmerged slices, lost ragged slice, whole-vocabulary
    cut at 256) is rejected by a named case;
  * contrast: on the peaked 151 936-token row of tests/test_gpu_ops.py::test_sample_token_gpu_matches_oracle, with that
    test's own parameters and u (six random draws and u = 0 for each of six parameter sets), 6 of the 12 mutants return the
    oracle's token at every draw: top-k keeping k - 1, ties from the highest index, the signed-zero key, the reciprocal
    temperature, and `>` for `>=` in the nucleus and in the draw.  Every one of the 12 is rejected here by a named case.
"""

from __future__ import annotations

import numpy as np
import pytest

from oracle import cpu_ref as O
from tests import sampling_ref as R


def test_case_table_reaches_every_launch_shape_and_switch():
    shapes = {g: {c.shape for c in cs} for g, cs in R.GROUPS.items()}
    every = {"sliced", "whole_row", "vocab_multinomial", "vocab_nucleus"}
    assert shapes["g1"] == every and {c.shape for c in R.GRADED} == every
    assert shapes["g2"] == {"sliced"} and shapes["g3"] == {"sliced", "whole_row"} and shapes["g4"] == {"vocab_nucleus"}
    assert shapes["g5"] == shapes["g6"] == {"sliced", "whole_row", "vocab_nucleus"}
    assert {c.shape for c in R.GROUPS["g7"] if c.rows[0].lead is not None} == {"sliced", "whole_row", "vocab_nucleus"}
    # both sides of the device-side decision, at both V, and rows of both kinds in one launch
    for c in R.GROUPS["g4"]:
        n = [int(R.kept_sets(r, c.k, c.p)[0].size) for r in c.rows]
        assert n[0] == int(c.name.rsplit("n", 1)[1]) and n[1] <= R.WHOLE_K
    # stage 2 sorts N = 2^ceil(log2 k) keys: rank sort up to 128, bitonic above
    assert {c.k for c in R.GROUPS["g2"]} == {1, 2, 127, 128, 129, 1023, 1024}
    # kept sets that cross an index byte
    for name, lo, hi in (("g5_index_bytes_sliced_k700", 65000, 65699), ("g5_index_bytes_whole_k1025", 65000, 66024),
                         ("g5_index_255_256_k80", 200, 279)):
        c = R.BY_NAME[name]
        K, Z = R.kept_sets(c.rows[0], c.k, c.p)
        assert (K[0], K[-1], K.size, Z.size) == (lo, hi, hi - lo + 1, 0)
    K, _ = R.kept_sets(R.Row(100), 10, 0.5)
    assert K.tolist() == [0, 1, 2, 3, 4]
    assert len(set(R.MUTANTS)) == 12 and set(R.REJECTED_BY) == set(R.MUTANTS)


@pytest.mark.parametrize("case", R.CASES, ids=str)
def test_precondition_exact_case(case):
    us = R.case_us(case)
    assert all(np.float32(u) == u and 0.0 <= u <= 1.0 for u in us) and us[0] == 0.0 and us[-1] == 1.0
    assert len(us) <= 64 * len(case.rows)
    t = np.float32(case.T)
    for row in case.rows:
        x = R.build_row(row)
        for dt in case.dtypes:
            np.testing.assert_array_equal(R.rounded(x, dt).view(np.uint32), x.view(np.uint32))
        top = np.float32(row.value) / t
        assert (top - np.float32(row.low) / t) >= 30.0                   # every other mass is exactly 0
        if row.lead is not None:
            a, b, r = np.float32(row.lead), np.float32(row.value), np.float32(1.0) / t
            assert a < b and np.nextafter(a, np.float32(np.inf)) == b and a / t == b / t and a * r != b * r
        K, Z = R.kept_sets(row, case.k, case.p)
        assert len(R.pick_js(K, row.V, 0)) <= 64
        prep = R.prepare(x, case.T, case.k, case.p)
        assert prep[1][-1] == float(K.size) * R.ONE                       # the restatement's kept mass is n * 2^32
        kept = np.sort(prep[0])
        np.testing.assert_array_equal(kept, np.sort(np.concatenate([K, Z])))
        for u in us:
            want = R.expected_token(K, Z, u)
            assert O.sample_token_u(x, case.T, case.k, case.p, u) == want == R.draw(prep, u), (row, u)
        # the midpoints alone read the whole mass-carrying kept set out when all of them are drawn
        if K.size <= 8:
            assert [R.expected_token(K, Z, float(np.float32((j + 0.5) / K.size))) for j in range(K.size)] == K.tolist()


@pytest.mark.parametrize("case", R.GRADED, ids=str)
def test_precondition_graded_case(case):
    x = R.build_graded(case)
    live = x[x > -100]
    assert live.max() - live.min() <= 6.0 and 3 <= np.unique(live).size <= 4
    us = R.graded_us(case)
    assert 2 <= len(us) <= 64 and all(np.float32(u) == u and 0.0 < u < 1.0 for u in us)
    prep = R.prepare(x, case.T, case.k, case.p)
    toks = set()
    for u in us:
        tok, margin = O.sample_token_u(x, case.T, case.k, case.p, u, return_margin=True)
        assert margin >= R.GRADED_MARGIN, (u, margin)
        assert tok == R.draw(prep, u)
        toks.add(tok)
    assert len(toks) == len(us)                                           # one draw per heavy token


def test_graded_rows_reach_both_sides_of_the_whole_vocabulary_decision():
    for c in R.GRADED:
        if c.shape != "vocab_nucleus":
            continue
        z = np.sort(R.build_graded(c).astype(np.float64) / c.T)[::-1]
        pr = np.exp(z - z[0])
        share = pr[:R.WHOLE_K].sum() / pr.sum()
        assert (share > c.p + 0.01) if "candidates" in c.name else (share < c.p - 0.01), (c.name, share)


@pytest.mark.parametrize("mut", R.MUTANTS)
def test_each_mutant_is_rejected_by_its_named_case(mut):
    named = {**R.BY_NAME, **{c.name: c for c in R.GRADED}}[R.REJECTED_BY[mut]]
    assert R.rejects(named, mut)


def test_mutants_of_one_branch_do_not_show_on_another():
    """The slice and whole-vocabulary mutants exist only on their launch shapes: a table without those shapes passes them."""
    assert not R.rejects(R.BY_NAME["g1_whole_k1025_V4097"], "slices_not_merged")
    assert not R.rejects(R.BY_NAME["g1_whole_k1025_ragged_V4200"], "ragged_slice_dropped")
    assert not R.rejects(R.BY_NAME["g4_decision_V8193_n256"], "vocab_nucleus_cut_256")
    assert not R.rejects(R.BY_NAME["g2_k127_p1.0"], "draw_gt")           # 127 is no power of two: no u sits on a boundary


def test_contrast_random_u_on_a_peaked_row_passes_most_mutants(capsys):
    """The existing test's row, parameters and u (test_sample_token_gpu_matches_oracle, float32): which mutants return the
    oracle's token at every one of its draws."""
    survivors = set(R.MUTANTS)
    for T, k, p in [(1.0, 0, 1.0), (0.7, 40, 1.0), (1.3, 0, 0.9), (0.8, 50, 0.95), (1.0, 1, 1.0), (2.0, 1000, 0.5)]:
        rng = np.random.default_rng(41)
        V = 151936
        lg = (rng.standard_normal(V) * 2.5).astype(np.float32)
        lg[rng.integers(0, V, 20)] += rng.uniform(4, 9, 20).astype(np.float32)
        us = []
        while len(us) < 6:
            u = float(np.float32(rng.random()))
            if O.sample_token_u(lg, T, k, p, u, return_margin=True)[1] > 1e-4:
                us.append(u)
        us.append(0.0)
        good = R.prepare(lg, T, k, p)
        want = [R.draw(good, u) for u in us]
        for mut in sorted(survivors):
            bad = R.prepare(lg, T, k, p, mut)
            if [R.draw(bad, u, mut) for u in us] != want:
                survivors.discard(mut)
    with capsys.disabled():
        print(f"\ncontrast: {len(survivors)} of {len(R.MUTANTS)} mutants pass the random-u test on the peaked row: {sorted(survivors)}")
    assert len(survivors) >= 6
