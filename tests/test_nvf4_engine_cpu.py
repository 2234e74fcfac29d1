"""CPU checks of the engine's NVF4 weights (weight_format "nvf4"): the NK-layout restatement against the reference
layout on hand-worked rows, bf16-exactness of every dequantised value, and the host-side validation of Engine's layer
dicts (no device touched)."""

from __future__ import annotations

import importlib

import numpy as np
import pytest

from tests import nvf4_engine_ref as NE
from tests import nvf4_ref as R


def hand_rows() -> tuple[np.ndarray, list[tuple[int, list[int]]]]:
    """Rows of K = 64, and per row the expected scale byte and leading data bytes of its first block.  The second block
    of every row is (12, 0, ...): scale 12 / 6 = 2.0 -> byte 0x40, and 12 / 2 = 6 -> code 7."""
    K = 64
    rows, want = [], []

    def row(first):
        r = np.zeros(K, np.float32)
        r[:len(first)] = first
        r[32] = 12.0
        return r

    rows.append(row([6.0, 1.25, -1.25, 0.25]))        # scale 1 (0x38): ties 1.25 -> 1.5 (3), -1.25 -> 11, 0.25 -> .5 (1)
    want.append((0x38, [0x37, 0x1B]))
    rows.append(row([np.nan, 3.0]))                     # NaN dropped from the max: scale 0.5 (0x30); NaN -> 7, 3 / .5 = 6 -> 7
    want.append((0x30, [0x77]))
    rows.append(row([np.inf, 1.0]))                     # inf: exponent and mantissa clamp (0x7F = 480); inf -> 7, 1/480 -> 0
    want.append((0x7F, [0x07]))
    rows.append(row([2.0 ** -28, -(2.0 ** -28)]))       # max under 1e-8: scale 1 (0x38), codes 0 and -0 (8)
    want.append((0x38, [0x80]))
    rows.append(row([2.0 ** -25, 2.0 ** -26]))          # max in (1e-8, 6e-8]: scale max/6 <= 1e-8 is not normalised -> 0x38
    want.append((0x38, [0x00]))
    return np.stack(rows), want


def test_nk_restatement_on_hand_worked_rows():
    w, want = hand_rows()
    data, scale = NE.quantize_nk(w)
    assert data.shape == (w.shape[0], 32) and scale.shape == (w.shape[0], 2)
    for i, (sb, first) in enumerate(want):
        assert scale[i, 0] == sb, (i, hex(scale[i, 0]))
        assert list(data[i, :len(first)]) == first, (i, [hex(b) for b in data[i, :len(first)]])
        assert not data[i, len(first):16].any()
        assert scale[i, 1] == 0x40 and data[i, 16] == 0x07 and not data[i, 17:].any()   # 12 = 6 x 2.0
    ref_data, ref_scale = NE.transposed_ref(w)
    np.testing.assert_array_equal(data, ref_data)
    np.testing.assert_array_equal(scale, ref_scale)


def test_nk_restatement_is_transposed_reference_on_random_rows():
    rng = np.random.default_rng(3)
    N, K = 37, 96
    w = NE.bf16_round(rng.standard_normal((N, K)).astype(np.float32) * np.exp2(rng.integers(-30, 12, (N, 1))).astype(np.float32))
    w[5, 40] = np.nan
    w[9, 3] = -np.inf
    data, scale = NE.quantize_nk(w)
    ref_data, ref_scale = NE.transposed_ref(w)
    np.testing.assert_array_equal(data, ref_data)
    np.testing.assert_array_equal(scale, ref_scale)
    # and the dequantised matrix is the reference's dequantisation, transposed
    np.testing.assert_array_equal(NE.dequant_nk(data, scale), R.dequant(ref_data.T, ref_scale.T, K).T)


def test_every_code_scale_product_is_exact_in_bf16():
    codes = np.arange(16)
    sbytes = np.arange(256)
    prod = (R.E2M1[codes][:, None] * R.scale_value(sbytes)[None, :]).astype(np.float32)
    assert prod.shape == (16, 256)
    np.testing.assert_array_equal(NE.bf16_round(prod), prod)
    assert np.isfinite(prod).all()


@pytest.mark.parametrize("module", ["pygpukit_amd.ops", "pygpukit_amd.ops.matmul", "pygpukit_amd.ops.matmul.nvf4"])
def test_nk_names_exported(module):
    mod = importlib.import_module(module)
    for n in ("quantize_bf16_to_nvf4_nk", "nvf4_nk_get_sizes", "quantize_nvf4_nk"):
        assert hasattr(mod, n), n
    assert mod.nvf4_nk_get_sizes(48, 4096) == (48 * 2048, 48 * 128)


class _Arr:
    """Stand-in for a GPUArray: Engine's host-side checks read only .dtype and .shape."""

    def __init__(self, shape, dtype):
        self.shape, self.dtype = tuple(shape), dtype


CFG = dict(vocab_size=512, hidden_size=256, num_layers=2, num_heads=4, num_kv_heads=2, head_dim=64, intermediate_size=512,
           norm_eps=1e-6, rope_theta=1e6)


def _nvf4_layers(cfg):
    from pygpukit_amd.core.dtypes import uint8
    from pygpukit_amd.llm.engine import linear_shapes

    out = []
    for _ in range(cfg["num_layers"]):
        lw = {}
        for name, (N, K) in linear_shapes(cfg).items():
            lw[name] = _Arr((N, K // 2), uint8)
            lw["s" + name[1:]] = _Arr((N, K // 32), uint8)
        out.append(lw)
    return out


def test_engine_layer_validation_accepts_nk_layout():
    from pygpukit_amd.llm.engine import check_nvf4_layers

    check_nvf4_layers(CFG, _nvf4_layers(CFG))


def test_engine_layer_validation_rejects_bad_layers():
    from pygpukit_amd.core.dtypes import bfloat16, uint8
    from pygpukit_amd.llm.engine import check_nvf4_layers

    cases = []
    lay = _nvf4_layers(CFG)
    lay[1]["w_o"] = _Arr(lay[1]["w_o"].shape, bfloat16)                    # wrong dtype of the codes
    cases.append((lay, "w_o must be uint8"))
    lay = _nvf4_layers(CFG)
    lay[0]["s_down"] = _Arr(lay[0]["s_down"].shape, bfloat16)              # wrong dtype of the scales
    cases.append((lay, "s_down must be uint8"))
    lay = _nvf4_layers(CFG)
    lay[0]["w_qkv"] = _Arr((lay[0]["w_qkv"].shape[1], lay[0]["w_qkv"].shape[0]), uint8)   # [K/2, N]: the reference layout
    cases.append((lay, "w_qkv must be uint8"))
    lay = _nvf4_layers(CFG)
    lay[0]["s_gate_up"] = _Arr((1024, 16), uint8)                          # [N, K/16]
    cases.append((lay, "s_gate_up must be uint8"))
    lay = _nvf4_layers(CFG)
    del lay[1]["s_qkv"]                                                    # missing scales
    cases.append((lay, "needs both w_qkv and s_qkv"))
    for layers, msg in cases:
        with pytest.raises(ValueError, match=msg):
            check_nvf4_layers(CFG, layers)
    with pytest.raises(ValueError, match="multiples of 128"):
        check_nvf4_layers(dict(CFG, hidden_size=192), _nvf4_layers(dict(CFG, hidden_size=192)))


def test_engine_rejects_nvf4_layers_before_the_device():
    from pygpukit_amd.core.dtypes import bfloat16
    from pygpukit_amd.llm.engine import Engine

    lay = _nvf4_layers(CFG)
    lay[0]["w_down"] = _Arr(lay[0]["w_down"].shape, bfloat16)
    with pytest.raises(ValueError, match="w_down must be uint8"):
        Engine(CFG, None, lay, None, weight_format="nvf4")
    with pytest.raises(ValueError, match="weight_format"):
        Engine(CFG, None, lay, None, weight_format="nvf3")
