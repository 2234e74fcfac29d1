"""group_norm / group_norm_silu on the GPU, element by element against the float64 oracle of tests/vae_ref.py on the inputs as the
device holds them, in both layouts and under both forced plans.

Bars (tests/test_dit_ops_gpu.py's), per element:
  float32:  FACTOR32 * yard, yard = the largest per-element error |ref32 - ref64| of a np.float32 two-pass restatement of the same
            case, computed here (a property of float32 and of the case, not of the kernel); never above 1e-4 * the case's scale.
  16-bit:   one ulp of the output dtype at |ref| (2^-7 |ref| bfloat16, 2^-10 |ref| float16) plus the float32 term.
FACTOR32 is the smallest power of two at least twice the worst ratio max|gpu - ref64| / yard measured on an MI355X over the
float32 cases of this file: MEASURED_RATIO, printed again by every test (run with -s).

The stable-statistics case (vae_ref.gn_stable_inputs): 100 + N(0, 1) in float32.  The two-pass restatement's yard is 1.2e-5 there; a
one-pass sum / sum of squares variance errs by 2.5e-3 (209 x the yard: test_vae_cpu.py::test_one_pass_variance_cannot_pass_the_
stable_case prints both on the same inputs), so FACTOR32 <= 32 lets the Welford / Chan kernel pass and no sum-of-squares kernel."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from tests import vae_ref as R

pytestmark = pytest.mark.gpu

MEASURED_RATIO = 1.543   # worst max|gpu - ref64| / yard over the float32 cases, measured on an MI355X (group_norm (1, 10, 4, 6, 2)
                         # NCHW; next (1, 6, 7, 9, 6) 1.318, (1, 32, 37, 31, 2) block 1.300; the 100 + N(0, 1) case 0.366);
                         # twice it is 3.086
FACTOR32 = 4.0
CAP32 = 1e-4
ULP = {"bfloat16": 2.0 ** -7, "float16": 2.0 ** -10}
DTYPES = ("float32", "bfloat16", "float16")
EPS = 1e-5


def _dev(a, dtype):
    from pygpukit_amd.core import from_numpy
    from pygpukit_amd.core.dtypes import as_dtype

    return from_numpy(np.ascontiguousarray(a, dtype=np.float32)).astype(as_dtype(dtype))


def _host(a):
    from pygpukit_amd.core.dtypes import float32

    return a.astype(float32).to_numpy()


@functools.lru_cache(maxsize=None)
def _case(i, dtype, silu):
    """i: index into GN_CASES, or -1 for the stable-statistics case.  -> inputs as held, ref64, ref32."""
    if i >= 0:
        groups = R.GN_CASES[i][4]
        x, gamma, beta = (R.round_to(a.astype(np.float64), dtype) for a in R.gn_inputs(i))
    else:
        groups = R.GN_STABLE_CASE[4]
        x, gamma, beta = (R.round_to(a.astype(np.float64), dtype) for a in R.gn_stable_inputs())
    ref64 = R.group_norm(x, gamma, beta, groups, EPS, silu=silu)
    ref32 = R.group_norm(x, gamma, beta, groups, EPS, silu=silu, dtype=np.float32)
    for a in (x, gamma, beta, ref64, ref32):
        a.setflags(write=False)
    return x, gamma, beta, groups, ref64, ref32


def _run(i, dtype, silu, channels_last, **kw):
    from pygpukit_amd.ops.nn.norm import group_norm, group_norm_silu

    x, gamma, beta, groups, _, _ = _case(i, dtype, silu)
    xd = _dev(x.transpose(0, 2, 3, 1) if channels_last else x, dtype)
    y = (group_norm_silu if silu else group_norm)(xd, _dev(gamma, dtype), _dev(beta, dtype), groups, EPS, channels_last=channels_last, **kw)
    h = _host(y)
    return h.transpose(0, 3, 1, 2) if channels_last else h


def _check(name, dtype, got, ref64, ref32, factor=FACTOR32):
    yard = float(np.abs(ref32.astype(np.float64) - ref64).max())
    cap = CAP32 * max(1.0, float(np.abs(ref64).max()))
    term32 = min(factor * yard, cap)
    err = np.abs(got.astype(np.float64) - ref64)
    bar = term32 if dtype == "float32" else ULP[dtype] * np.abs(ref64) + term32
    worst = float((err / np.maximum(bar, 1e-300)).max())
    ratio = float(err.max() / yard) if yard > 0 else 0.0
    print(f"{name} {dtype}: max err {err.max():.3e}, yard {yard:.3e}" + (f", ratio {ratio:.3f}" if dtype == "float32" else "") +
          f", worst err / bar {worst:.3f}")
    assert np.isfinite(got).all() and got.shape == ref64.shape and yard > 0
    assert (err <= bar).all(), f"{name} {dtype}: {int((err > bar).sum())} elements over the bar, worst err / bar {worst:.3f}"


@pytest.mark.parametrize("plan", ("block", "split"))
@pytest.mark.parametrize("channels_last", (False, True), ids=("nchw", "nhwc"))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("i", range(len(R.GN_CASES)), ids=[str(c) for c in R.GN_CASES])
def test_group_norm_matches_the_oracle(i, dtype, channels_last, plan, monkeypatch):
    from pygpukit_amd.ops.nn.norm import group_norm_plan

    n, c, h, w, g = R.GN_CASES[i]
    assert group_norm_plan(n, c, h * w, g, dtype, channels_last) == "block"          # every case is below the split threshold
    monkeypatch.setenv("PGK_GN_SPLIT", "1" if plan == "split" else "0")
    assert group_norm_plan(n, c, h * w, g, dtype, channels_last) == plan
    for silu in (False, True):
        _, _, _, _, ref64, ref32 = _case(i, dtype, silu)
        _check(f"group_norm{'_silu' if silu else ''} {R.GN_CASES[i]} {plan} cl={channels_last}", dtype,
               _run(i, dtype, silu, channels_last), ref64, ref32)


def test_group_norm_plan_without_a_switch(monkeypatch):
    from pygpukit_amd.ops.nn.norm import group_norm_plan

    monkeypatch.delenv("PGK_GN_SPLIT", raising=False)
    assert group_norm_plan(1, 128, 1024 * 1024, 32, "bfloat16", True) == "split"      # 4 channels x 1M pixels
    assert group_norm_plan(1, 512, 128 * 128, 32, "bfloat16", True) == "split"
    assert group_norm_plan(2, 32, 16 * 16, 4) == "block"


@pytest.mark.parametrize("channels_last", (False, True), ids=("nchw", "nhwc"))
@pytest.mark.parametrize("dtype", ("float32", "bfloat16"))
def test_group_norm_split_plan_is_run_to_run_identical(dtype, channels_last, monkeypatch):
    """Cases 4 and 5: three (512, 512, 123 pixels) and four chunks per group - case 5 in bfloat16 channels-last on the row form -
    merged in a fixed order, no atomics."""
    monkeypatch.setenv("PGK_GN_SPLIT", "1")
    for i in (4, 5):
        a, b = _run(i, dtype, True, channels_last), _run(i, dtype, True, channels_last)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("plan", ("block", "split"))
@pytest.mark.parametrize("channels_last", (False, True), ids=("nchw", "nhwc"))
def test_group_norm_statistics_are_stable_at_a_large_mean(channels_last, plan, monkeypatch):
    assert FACTOR32 <= 32
    monkeypatch.setenv("PGK_GN_SPLIT", "1" if plan == "split" else "0")
    _, _, _, _, ref64, ref32 = _case(-1, "float32", False)
    _check(f"group_norm 100 + N(0,1) {plan} cl={channels_last}", "float32", _run(-1, "float32", False, channels_last), ref64, ref32)


def test_group_norm_out_is_honoured_and_may_alias_the_input():
    from pygpukit_amd.ops.nn.norm import group_norm_silu

    x, gamma, beta, groups, ref64, ref32 = _case(3, "float32", True)
    xd = _dev(x, "float32")
    assert group_norm_silu(xd, _dev(gamma, "float32"), _dev(beta, "float32"), groups, EPS, out=xd) is xd
    _check("group_norm_silu in place", "float32", _host(xd), ref64, ref32)
