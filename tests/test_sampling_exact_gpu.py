"""Exact checks of csrc/ops_sampling.hip on the rows of tests/sampling_ref.py: the kept set is read out of the kernels
token by token, on all four launch shapes (sliced top-k, whole-row, whole-vocabulary multinomial, whole-vocabulary
nucleus on both sides of its device-side decision).

On a plateau row every kept token has the integer mass 2^32 and every other token the mass 0, on the device as in the
oracle, so u = (j + 0.5) / n must return the j-th kept index and u = j / n (n a power of two) the (j - 1)-th: index-exact,
no margin, no skipped draw.  Every row of a launch is checked at every u of the launch.  Only the graded rows lean on a
margin (each draw 5e-4 of the kept mass from a boundary) and only the engine's cross-check against the oracle skips a
draw (those within 1e-4); its comparison with pgk_sample_token on the engine's own logits is bit-exact.
tests/test_sampling_exact_cpu.py proves the expectations against the oracle and shows which errors the cases reject.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from oracle import cpu_ref as O
from tests import sampling_ref as R
from tests.golden_cfg import TINY

pytestmark = pytest.mark.gpu


def _dev(x: np.ndarray, dtype: str):
    from pygpukit_amd.core import from_numpy

    x = np.ascontiguousarray(x, dtype=np.float32)
    if dtype == "f32":
        return from_numpy(x)
    return from_numpy(x.astype(np.float16) if dtype == "f16" else O.f32_to_bf16_bits(x).reshape(x.shape))


def _sample(d, rows, V, T, k, p, u, res, u_buf=None) -> np.ndarray:
    from pygpukit_amd import _hip

    res.copy_from_numpy(np.full(rows, -7, np.int32))                       # every row must be written
    _hip.call("pgk_sample_token", d._p, rows, V, d.dtype.code, C.c_float(T), int(k), C.c_float(p), C.c_float(u),
              u_buf._p if u_buf is not None else None, res._p, None)
    return res.to_numpy().copy()


def _run_exact(case: R.Case, dtype: str) -> None:
    import pygpukit_amd as pk
    from pygpukit_amd import ops
    from pygpukit_amd.core import from_numpy

    x = np.stack([R.build_row(r) for r in case.rows])
    rows, V = x.shape
    d, res, ub = _dev(x, dtype), pk.empty((rows,), "int32"), from_numpy(np.zeros(1, np.float32))
    sets = [R.kept_sets(r, case.k, case.p) for r in case.rows]
    bad = []
    for u in R.case_us(case):
        want = np.array([R.expected_token(K, Z, u) for K, Z in sets])
        got = {"value": _sample(d, rows, V, case.T, case.k, case.p, u, res)}
        ub.copy_from_numpy(np.array([u], np.float32))
        got["u_buf"] = _sample(d, rows, V, case.T, case.k, case.p, 0.25, res, ub)
        if case.k > 0 and case.p == 1.0:
            res.copy_from_numpy(np.full(rows, -7, np.int32))
            ops.sample_topk_to_buf_ptr(d, res, ub, case.k, case.T)
            got["to_buf_ptr"] = res.to_numpy().copy()
        bad += [(form, r, u, int(g[r]), int(want[r])) for form, g in got.items() for r in range(rows) if g[r] != want[r]]
    assert not bad, f"{case.name} {dtype} ({case.shape}): {len(bad)} wrong draws (form, row, u, got, want): {bad[:8]}"


def _params(groups):
    return [pytest.param(c, dt, id=f"{c.name}-{dt}") for g in groups for c in R.GROUPS[g] for dt in c.dtypes]


@pytest.mark.parametrize("case,dtype", _params(["g1"]))
def test_launch_shapes_enumerate_the_kept_set(case, dtype):
    """Group 1: every launch shape by (k, V) - one slice, a ragged last slice (of one token too), three slices, the
    whole-row kernel (k = 1025, k >= V, tiny rows), whole-vocabulary multinomial and nucleus; several rows per launch."""
    _run_exact(case, dtype)


@pytest.mark.parametrize("case,dtype", _params(["g2"]))
def test_top_k_at_the_sort_switch(case, dtype):
    """Group 2: k = 1, 2, 127, 128 (rank sort), 129, 1023, 1024 (bitonic sort), p = 1 and p = 0.5; at k = 2 and 128 the
    nucleus target is exactly the mass of half the tokens and u = j / k sits exactly on the draw's boundaries."""
    _run_exact(case, dtype)


@pytest.mark.parametrize("case,dtype", _params(["g3", "g4", "g5"]))
def test_nucleus_base_whole_vocabulary_decision_and_index_bytes(case, dtype):
    """Group 3: the nucleus is cut within what top-k kept (10 of 100 equal tokens, p = 0.5 -> 5).  Group 4: all-equal rows
    that need 255 / 256 tokens (candidate kernel) and 257 / 300 (whole-row kernel), next to a row that always ends in the
    candidate kernel.  Group 5: ties whose kept set crosses index 65536 and 256 (the low-word radix passes)."""
    _run_exact(case, dtype)


@pytest.mark.parametrize("case,dtype", _params(["g6"]))
def test_signed_zeros_are_one_value(case, dtype):
    """Group 6: a plateau of -0.0 and +0.0 mixed; the top-k and the nucleus boundary inside it are by index alone.  (These
    cases found smp_key ordering -0.0 below +0.0: every one of them kept the positive zeros first until the key was fixed.)"""
    _run_exact(case, dtype)


@pytest.mark.parametrize("case,dtype", _params(["g7"]))
def test_temperature_is_a_division(case, dtype):
    """Group 7: adjacent floats a < b with fl(a / T) == fl(b / T), a at the lower index: the contract keeps a at the k-th
    place, a multiplication by fl(1 / T) keeps b.  And cases of groups 1, 2 and 6 again at T = 0.7, in every dtype."""
    _run_exact(case, dtype)


@pytest.mark.parametrize("case", R.GRADED, ids=str)
def test_graded_rows_match_the_oracle(case):
    """Group 9: three or four levels within 6 of the maximum; u at the midpoint of every token that owns at least 1e-3 of
    the kept mass (5e-4 from a boundary, asserted on the CPU).  No draw is skipped."""
    import pygpukit_amd as pk

    x = R.build_graded(case)
    d, res = _dev(x[None], "f32"), pk.empty((1,), "int32")
    bad = []
    for u in R.graded_us(case):
        want = O.sample_token_u(x, case.T, case.k, case.p, u)
        got = int(_sample(d, 1, x.size, case.T, case.k, case.p, u, res)[0])
        if got != want:
            bad.append((u, got, want))
    assert not bad, f"{case.name} ({case.shape}): {len(bad)} wrong draws (u, got, want): {bad[:8]}"


# (T, top_k, top_p, whole-vocabulary nucleus ends in the candidate kernel).  The random model's logits have a standard
# deviation of about 0.3: the temperatures make the rows peaked enough that most draws are 1e-4 clear of a boundary.
ENGINE_SETS = [(0.25, 40, 0.95, None), (0.1, 0, 1.0, None), (0.25, 0, 0.9, False), (0.1, 2000, 1.0, None), (0.05, 0, 0.9, True)]


def test_engine_draws_on_every_launch_shape(monkeypatch, capsys):
    """The captured decode step at V = 3 * 4096 + 37 (multi-slice scratch, ragged last slice), 19 sequences stepped in two
    chunks (16 + 3: the second chunk reads u_ring + 16), a ring of 3 rows wrapped by 5 steps, and parameter sets for the four
    launch shapes (top_p = 0.9 falls through to the whole-row kernel at T = 0.25, where the 256 best tokens hold well under
    0.9 of the mass, and ends in the candidate kernel at T = 0.05).  Every token equals pgk_sample_token on the step's own
    fp32 logits with the same u - bit-exact, same code on same data - and the oracle's wherever the oracle's margin exceeds
    1e-4."""
    import pygpukit_amd as pk
    from pygpukit_amd.llm import synthetic as S

    monkeypatch.setenv("PGK_BATCHED_MAX", "16")
    cfg = dict(TINY, vocab_size=3 * R.SLICE + 37)
    V, B, ring, steps = cfg["vocab_size"], 19, 3, 5
    rng = np.random.default_rng(77)
    prompts = [[int(t) for t in rng.integers(0, V, int(rng.integers(1, 9)))] for _ in range(B)]
    eng = S.build_engine_from_weights(cfg, S.make_qwen3_weights(cfg, seed=19), max_seq_len=32, max_batch=B)
    first = [int(np.argmax(eng.prefill(p, seq=b))) for b, p in enumerate(prompts)]
    res = pk.empty((1,), "int32")
    checked = total = 0
    shares = {}
    for T, k, p, in_candidates in ENGINE_SETS:
        u = rng.random((ring, B), dtype=np.float32)
        eng.set_sampling(T, top_k=k, top_p=p, uniforms=u)
        eng.set_state(first, [len(pr) for pr in prompts])
        eng.capture(B)
        eng.reset_log()
        for s in range(steps):
            eng.replay(1)
            eng.synchronize()
            lg = eng.logits(B).to_numpy().copy()
            toks = eng.read_tokens(B, s + 1)[s]
            if in_candidates is not None:                                   # which side of the device-side decision the rows are on
                pr = np.exp(np.sort(lg.astype(np.float64) / T, axis=1)[:, ::-1] - lg.max(axis=1, keepdims=True) / T)
                share = pr[:, :R.WHOLE_K].sum(axis=1) / pr.sum(axis=1)
                shares[T] = (float(share.min()), float(share.max()))
                assert (share > p + 0.02).all() if in_candidates else (share < p - 0.02).all(), (T, p, shares[T])
            for b in range(B):
                ub = float(u[s % ring, b])
                same = int(_sample(_dev(lg[b:b + 1], "f32"), 1, V, T, k, p, ub, res)[0])
                assert int(toks[b]) == same, (T, k, p, s, b, ub, int(toks[b]), same)
                want, margin = O.sample_token_u(lg[b], T, k, p, ub, return_margin=True)
                total += 1
                if margin > 1e-4:
                    assert same == want, (T, k, p, s, b, ub, same, want, margin)
                    checked += 1
    eng.set_sampling(0.0)
    with capsys.disabled():
        print(f"\nengine sampling: {checked} of {total} draws ({checked / total:.1%}) are more than 1e-4 from a boundary and match the oracle;"
              f" mass share of the 256 best tokens by temperature (min, max): {shares}")
    assert checked * 2 >= total
