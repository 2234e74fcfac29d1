"""FP8 KV cache without a GPU: the oracle's quantiser against its own table, and the host-only plan helper."""

from __future__ import annotations

import numpy as np
import pytest

from oracle import cpu_ref as O
from tests import kv_fp8_ref as R

SCALES = np.array([0.37, 1.9], np.float32)


def test_quantise_inverts_dequantise_on_every_finite_code():
    codes = np.array([c for c in range(256) if c not in (0x7F, 0xFF)], np.uint8)
    grid = np.broadcast_to(codes[:, None, None], (254, 2, 1))                     # [S, Hkv, D]: every code under both scales
    values = R.dequantise(grid, SCALES, head_axis=1)
    np.testing.assert_array_equal(R.quantise(values, SCALES), grid)
    assert R.quantise(np.float32(-0.0).reshape(1, 1, 1), [1.0])[0, 0, 0] == 0x80


def test_quantise_saturates_at_448_scales():
    x = np.array([[[448.0, 449.0, 1e30, np.inf]], [[-448.0, -449.0, -1e30, -np.inf]]], np.float32) * 1.9        # [2, 1, 4]
    np.testing.assert_array_equal(R.quantise(x, [1.9]), np.array([[[0x7E] * 4], [[0xFE] * 4]], np.uint8))
    assert O.fp8_e4m3_table()[0x7E] == 448.0


def test_plan_accepts_and_rejects():
    from pygpukit_amd import _hip
    from pygpukit_amd.ops.nn import sdpa_kv_fp8_plan

    try:
        _hip.load()
    except (RuntimeError, OSError) as e:
        pytest.skip(f"libpgk_hip.so does not load here: {e}")
    assert sdpa_kv_fp8_plan(32, 8, 128, 64, "bfloat16") == ("kv_fp8_split", 1)
    assert sdpa_kv_fp8_plan(8, 2, 64, 600, "float16") == ("kv_fp8_split", 3)
    assert sdpa_kv_fp8_plan(3, 3, 128, 131072, "bfloat16") == ("kv_fp8_split", 64)
    for bad in ((8, 3, 128, 64, "bfloat16", True), (8, 2, 96, 64, "bfloat16", True), (8, 2, 128, 0, "bfloat16", True),
                (8, 2, 128, 64, "float32", True), (8, 2, 128, 64, "bfloat16", False)):
        with pytest.raises(ValueError, match="pgk_sdpa_kv_fp8_plan"):
            sdpa_kv_fp8_plan(*bad)
