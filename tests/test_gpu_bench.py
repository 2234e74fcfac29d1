"""bench.py as a program: a plain run measures the headline and nothing else, `--full` adds every other leg after it, and
the headline path (result line fields, dumped arrays) is the same in both.  Two layers (`--layers`, result marked INVALID)
and a handful of steps: what is checked is which legs run, not a figure."""

from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADLINE_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}
FULL_KEYS = {"roofline", "roofline_kernels", "prefill", "prefill_long", "extras", "cpu_baseline"}
STEPS, WARMUP = 4, 2
SMALL_FULL = ["--full", "--config4-steps", "4", "--no-config5", "--long-prefill", "256", "--cpu-decode-tokens", "1"]


def _run(out_dir: str, extra: list[str]) -> dict:
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
           "--layers", "2", "--dump-outputs", out_dir] + extra
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.splitlines()
    assert len(lines) == 1, p.stdout[:2000]          # ONE JSON line on stdout, whatever else the run does
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bench")
    plain_dir, full_dir = str(d / "plain"), str(d / "full")
    return {"plain": _run(plain_dir, []), "full": _run(full_dir, SMALL_FULL), "plain_dir": plain_dir, "full_dir": full_dir}


@pytest.mark.gpu
def test_plain_run_reports_the_headline_and_runs_no_other_leg(runs):
    r = runs["plain"]
    assert HEADLINE_KEYS <= set(r)
    assert r["full"] is False
    assert not FULL_KEYS & set(r), sorted(FULL_KEYS & set(r))
    assert "sum_of_kernel_us" not in r["step_roofline"]      # the per-kernel events belong to --full
    assert (r["unit"], r["higher_is_better"], r["dtype"], r["steps"], r["warmup"]) == ("tokens/s", True, "bf16", STEPS, WARMUP)
    assert r["value"] * r["ms_per_step"] == pytest.approx(1000.0, rel=1e-9)   # one sequence: value = K / wall, ms_per_step = wall / K


@pytest.mark.gpu
def test_full_run_adds_every_other_leg(runs):
    r = runs["full"]
    assert HEADLINE_KEYS <= set(r) and FULL_KEYS <= set(r)
    assert r["full"] is True
    assert r["metric"] == runs["plain"]["metric"] and r["config"] == runs["plain"]["config"]
    assert r["roofline"]["us_per_launch"] > 0 and len(r["roofline_kernels"]) >= 5
    assert r["step_roofline"]["sum_of_kernel_us"] > 0
    assert r["prefill"]["ms"] > 0 and r["prefill_long"]["tokens"] == 256
    assert {"config4", "config3_ctx2048_w8a16", "ctx2048_bf16"} <= set(r["extras"])
    assert "config5_llama8b_prefill4096" not in r["extras"]   # --no-config5 still trims a --full run
    assert r["cpu_baseline"]["value"] > 0


@pytest.mark.gpu
def test_full_does_not_change_what_the_headline_computes(runs):
    """The extra legs run after the timed steps and after the dump: the same tokens and bit-identical logits either way."""
    for name, shape in (("tokens.npy", (WARMUP + STEPS, 1)), ("logits.npy", (1, 151936))):
        a, b = (np.load(os.path.join(runs[k], name)) for k in ("plain_dir", "full_dir"))
        assert a.shape == shape and b.shape == shape
        assert np.array_equal(a, b), name
    assert runs["plain"]["first_tokens"] == runs["full"]["first_tokens"]
