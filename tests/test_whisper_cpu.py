"""conv1d, sdpa_noncausal and the Whisper encoder without a GPU: the NumPy oracle (tests/whisper_ref.py) against the reference's
recorded float32 CPU results (tests/golden/g10_whisper.npz), the proof that the GPU tests' bars separate right from wrong, the
exported surface, the C ABI of the new entry points, the host-only plan query and the argument checks (which run before
anything touches a device)."""

from __future__ import annotations

import os
import re

import numpy as np
import pytest

from pygpukit_amd import _hip
from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import bfloat16, float16, float32, int32
from pygpukit_amd.ops.conv import conv1d, conv1d_pack_weight, conv1d_plan
from pygpukit_amd.ops.nn.attention import sdpa_noncausal, sdpa_noncausal_strided
from tests import whisper_ref as R
from tests.conftest import ROOT, load_golden, rel_err

g10 = load_golden("g10_whisper.npz")
NEW_ENTRIES = ("pgk_conv1d", "pgk_conv1d_plan", "pgk_conv1d_packed_elems", "pgk_conv1d_pack_weight", "pgk_sdpa_noncausal")


# ---- oracle against the fixture -------------------------------------------------------------------------------------
# The fixture is float32 arithmetic in another summation order; the bars are a few float32 ulps of the largest partial sums
# (|conv| <= 8, |encoder output| <= 4): 2e-6 absolute, 2e-6 relative for the encoder (measured distances: 1e-6, 4.7e-7).
def _conv_fixture(i):
    case = tuple(int(v) for v in g10[f"c{i}_case"])
    b = g10[f"c{i}_b"] if f"c{i}_b" in g10.files else None
    return case, g10[f"c{i}_x"], g10[f"c{i}_w"], b, g10[f"c{i}_out"]


@pytest.mark.parametrize("i", range(len(R.FIXTURE_CONV)))
def test_conv1d_oracle_matches_the_reference(i):
    case, x, w, b, want = _conv_fixture(i)
    assert case == R.FIXTURE_CONV[i] and want.shape == (case[0], case[2], R.conv_out_length(case[3], case[4], case[5], case[6]))
    got = R.conv1d(x, w, b, case[5], case[6], dtype=np.float32)
    assert got.dtype == np.float32
    assert np.max(np.abs(got - want)) <= 2e-6
    assert np.max(np.abs(R.conv1d(x, w, b, case[5], case[6]) - want)) <= 2e-6


def test_attention_oracle_matches_the_reference():
    q, k, v, want = (g10[n] for n in ("a_q", "a_k", "a_v", "a_out"))
    assert q.shape[1] != k.shape[1] and want.shape == q.shape
    assert np.max(np.abs(R.sdpa_noncausal(q, k, v, dtype=np.float32) - want)) <= 2e-6
    assert np.max(np.abs(R.sdpa_noncausal(q, k, v) - want)) <= 2e-6


def test_encoder_oracle_matches_the_reference():
    cfg = R.fixture_config()
    tensors = R.make_weights(cfg, int(g10["enc_seed"]))
    assert "model.encoder.layers.0.self_attn.k_proj.bias" not in tensors
    assert g10["enc_mel"].shape == (1, 16, 74) and g10["enc_out"].shape == (1, 37, 128)
    got32 = R.encoder_forward(cfg, tensors, g10["enc_mel"], np.float32)
    assert got32.dtype == np.float32
    assert rel_err(got32, g10["enc_out"]) <= 2e-6
    assert rel_err(g10["enc_out"], R.encoder_forward(cfg, tensors, g10["enc_mel"])) <= 2e-6


# ---- the bars separate right from wrong -------------------------------------------------------------------------------
def conv_bar(case, x, w, b, ref, out_eps, factor=1.0):
    """tests/test_conv1d_gpu.py's elementwise bar: n 2^-24 (sum |x w| + |b|) for any fp32 summation order of n = C_in K + 1
    terms (x factor 2 for fp32 products), plus the output rounding out_eps |ref|."""
    n = case[1] * case[4] + 1
    return factor * n * 2.0 ** -24 * R.conv1d(x, w, b, case[5], case[6], absolute=True) + out_eps * np.abs(ref)


@pytest.mark.parametrize("case", R.CONV_CASES, ids=str)
def test_every_planted_conv_error_moves_the_output_far_beyond_the_bar(case):
    x, w, b = R.make_conv_case(case)
    right = R.conv1d(x, w, b, case[5], case[6])
    widest = float(conv_bar(case, x, w, b, right, 2.0 ** -8, 2.0).max())          # bf16 output, factor 2: the widest bar used
    for m in R.CONV_MUTATIONS:
        if m == "ignore_stride" and case[5] == 1:
            continue
        moved = float(np.max(np.abs(R.conv1d(x, w, b, case[5], case[6], mutate=m) - right)))
        assert moved >= 25 * widest, (m, moved, widest)


def visibility_case(hq, hkv, q_len, kv_len, d, j_star):
    """Q = 0, V zero except row j_star = 1: every probability is exactly 1 / kv_len and so is every output element."""
    q, k, _ = R.make_attn_case((hq, hkv, q_len, kv_len, d))
    v = np.zeros((hkv, kv_len, d), np.float32)
    v[:, j_star] = 1.0
    return np.zeros_like(q), k, v


@pytest.mark.parametrize("kv_len", [65, 200])
def test_every_planted_attention_error_is_caught_by_the_visibility_check(kv_len):
    """The GPU check is |out - 1/kv_len| <= eps / kv_len with eps = 2^-8 (bf16) or 2^-11 (f16), the output rounding.  A dropped
    key gives 0 and a causal mask 1/(i+1) or 0 on early rows: 256 bars away and more.  One padded key gives 1/(kv_len + 1):
    256 / (kv_len + 1) bars away in bf16 - 3.9 at 65 keys, 1.27 at 200, small but beyond the bar - and 8 times that in f16."""
    q_len = 70
    for j_star in (0, 63, 64, kv_len - 1):
        q, k, v = visibility_case(2, 2, q_len, kv_len, 64, j_star)
        right = R.sdpa_noncausal(q, k, v)
        assert np.max(np.abs(right - 1.0 / kv_len)) <= 1e-15
        bar = 2.0 ** -8 / kv_len
        padded = R.sdpa_noncausal(q, k, v, mutate="extra_padded_key")
        assert np.min(np.abs(padded - right)) >= 1.25 * bar and np.min(np.abs(padded - right)) >= 10 * 2.0 ** -11 / kv_len
        causal = R.sdpa_noncausal(q, k, v, mutate="causal")
        assert np.max(np.abs(causal - right)) >= 100 * bar
    q, k, v = visibility_case(2, 2, q_len, kv_len, 64, kv_len - 1)
    assert np.min(np.abs(R.sdpa_noncausal(q, k, v, mutate="drop_last_key") - 1.0 / kv_len)) >= 256 * bar


@pytest.mark.parametrize("shape", R.ATTN_SHAPES, ids=str)
def test_dropped_key_and_causal_mask_move_random_attention_beyond_the_bar(shape):
    """rel_err <= 1e-2 is the GPU bar; one padded key moves a random case by less than that - the visibility check above is
    what catches it."""
    q, k, v = R.make_attn_case(shape)
    right = R.sdpa_noncausal(q, k, v)
    for m in ("drop_last_key", "causal"):
        assert rel_err(R.sdpa_noncausal(q, k, v, mutate=m), right) >= 2e-2, m


def test_unknown_mutations_are_rejected():
    x, w, b = R.make_conv_case(R.CONV_CASES[0])
    with pytest.raises(ValueError):
        R.conv1d(x, w, b, mutate="swap")
    with pytest.raises(ValueError):
        R.sdpa_noncausal(*R.make_attn_case(R.ATTN_SHAPES[0]), mutate="swap")


# ---- exported surface -------------------------------------------------------------------------------------------------
def test_names_importable_where_the_reference_has_them():
    import pygpukit_amd
    from pygpukit_amd import asr, ops
    from pygpukit_amd.asr import whisper
    from pygpukit_amd.ops import basic, conv, nn

    assert ops.conv1d is conv.conv1d is conv1d and "conv1d" in ops.__all__
    assert conv.conv1d_plan is conv1d_plan and conv.conv1d_pack_weight is conv1d_pack_weight
    for mod in (nn, ops, basic, pygpukit_amd):
        assert mod.sdpa_noncausal is sdpa_noncausal and mod.sdpa_noncausal_strided is sdpa_noncausal_strided
    assert "sdpa_noncausal" in nn.__all__ and "sdpa_noncausal_strided" in nn.__all__ and len(set(nn.__all__)) == len(nn.__all__)
    for name in ("WhisperConfig", "WhisperWeights", "WhisperEncoder", "WhisperEncoderLayer", "create_encoder"):
        assert getattr(whisper, name) is getattr(asr, name) and name in whisper.__all__


def test_whisper_config_and_weights():
    from pygpukit_amd.asr.whisper import WHISPER_CONFIGS, WhisperConfig, WhisperWeights

    c = WhisperConfig()
    assert (c.d_model, c.encoder_layers, c.encoder_attention_heads, c.num_mel_bins, c.max_source_positions) == (1280, 32, 20, 128, 1500)
    assert c.head_dim == 64 and all(v.head_dim == 64 for v in WHISPER_CONFIGS.values())
    d = c.to_dict()
    assert d["encoder_ffn_dim"] == 5120 and "model_name_or_path" not in d
    c2 = WhisperConfig.from_dict({**d, "d_model": 384, "encoder_attention_heads": 6, "_name_or_path": "x/y", "not_a_field": 1})
    assert c2.d_model == 384 and c2.head_dim == 64 and c2.model_name_or_path == "x/y" and c2.to_dict() == {**d, "d_model": 384, "encoder_attention_heads": 6}
    cfg = R.fixture_config()
    tensors = R.make_weights(cfg, 3)
    w = WhisperWeights.from_tensors(cfg, tensors)
    assert w.encoder_conv1_weight.shape == (128, 16, 3) and w.encoder_conv2_weight.shape == (128, 128, 3)
    assert w.encoder_embed_positions.shape == (37, 128) and len(w.encoder_layers) == 2
    layer = w.encoder_layers[1]
    assert layer["self_attn_k_bias"] is None and layer["self_attn_q_bias"].shape == (128,) and layer["fc1_weight"].shape == (256, 128)
    assert set(layer) == {"self_attn_q_weight", "self_attn_q_bias", "self_attn_k_weight", "self_attn_k_bias", "self_attn_v_weight",
                          "self_attn_v_bias", "self_attn_out_weight", "self_attn_out_bias", "self_attn_layer_norm_weight",
                          "self_attn_layer_norm_bias", "fc1_weight", "fc1_bias", "fc2_weight", "fc2_bias", "final_layer_norm_weight",
                          "final_layer_norm_bias"}
    del tensors["model.encoder.layers.0.fc2.bias"]
    with pytest.raises(KeyError, match="fc2.bias"):
        WhisperWeights.from_tensors(cfg, tensors)


# ---- C ABI ------------------------------------------------------------------------------------------------------------
def _header_prototypes() -> dict:
    text = open(os.path.join(ROOT, "include", "pgk_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(2): (m.group(1).strip(), [a.strip() for a in m.group(3).split(",")])
            for m in re.finditer(r"\b(pgk_status|int|size_t)\s+(pgk_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def _ctype_of(arg: str):
    import ctypes as C

    if "*" in arg or arg.startswith("pgk_stream"):
        return C.c_void_p
    kind = arg.rsplit(" ", 1)[0]
    return {"int": C.c_int, "float": C.c_float, "int64_t": C.c_int64, "size_t": C.c_size_t, "pgk_dtype": C.c_int}[kind]


def test_header_prototypes_and_exports_agree_for_the_new_entries():
    import ctypes as C

    protos = _header_prototypes()
    lib = _hip.load()
    for name in NEW_ENTRIES:
        ret, args = protos[name]
        if ret == "pgk_status":
            argtypes, restype = _hip._PROTOS[name], C.c_int
        else:
            argtypes, restype = _hip._NON_STATUS[name]
            assert restype is {"int": C.c_int, "size_t": C.c_size_t}[ret]
        assert [_ctype_of(a) for a in args] == list(argtypes), name
        assert name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert protos["pgk_sdpa_noncausal"][1] == protos["pgk_sdpa_causal"][1]                  # the argument list of pgk_sdpa_causal


# ---- plan query (host only) -------------------------------------------------------------------------------------------
def test_plan_default(monkeypatch):
    monkeypatch.delenv("PGK_CONV_MFMA", raising=False)
    for case in R.CONV_CASES + ((1, 128, 1280, 3000, 3, 1, 1), (1, 1280, 1280, 3000, 3, 2, 1)):
        _, c_in, c_out, length, k, stride, padding = case
        assert conv1d_plan(c_in, c_out, length, k, stride, padding, float32) == "fma"
        for dt in (bfloat16, float16, "bfloat16"):
            assert conv1d_plan(c_in, c_out, length, k, stride, padding, dt) == "mfma"
    # slab + weight tile beyond the 64 KiB of LDS: (63 stride + K + 64 K) * 80 bytes
    assert conv1d_plan(8, 8, 5000, 12, 1, 0, bfloat16) == "fma" and conv1d_plan(8, 8, 5000, 11, 1, 0, bfloat16) == "mfma"
    assert conv1d_plan(8, 8, 5000, 3, 10, 0, float16) == "fma" and conv1d_plan(8, 8, 5000, 3, 9, 0, float16) == "mfma"


def test_plan_switch_forces_fma(monkeypatch):
    monkeypatch.setenv("PGK_CONV_MFMA", "0")
    for dt in (float32, bfloat16, float16):
        assert conv1d_plan(16, 32, 64, 3, 1, 1, dt) == "fma"
    monkeypatch.setenv("PGK_CONV_MFMA", "1")
    assert conv1d_plan(16, 32, 64, 3, 1, 1, bfloat16) == "mfma"


@pytest.mark.parametrize("args", [(0, 8, 9, 3, 1, 0), (8, 0, 9, 3, 1, 0), (8, 8, 0, 3, 1, 0), (8, 8, 9, 0, 1, 0), (8, 8, 9, 3, 0, 0),
                                  (8, 8, 9, 3, 1, -1), (8, 8, 2, 3, 1, 0), (8, 8, 9, 12, 2, 1)], ids=str)
def test_plan_rejects_bad_shapes(args):
    with pytest.raises(ValueError):
        conv1d_plan(*args, bfloat16)


def test_plan_rejects_bad_dtype():
    with pytest.raises(ValueError):
        conv1d_plan(8, 8, 9, 3, 1, 0, int32)


# ---- argument checks: ValueError before any device call -----------------------------------------------------------------
def _fake(shape, dtype=float32):
    return GPUArray(shape, dtype, device_ptr=0x1000, owns_memory=False)     # never dereferenced: the checks come first


BAD_CONV = [
    ("in_channels", dict(weight=_fake((8, 5, 3)))),                                        # C_in mismatch
    ("L_out", dict(input=_fake((1, 4, 2)), padding=0)),                                              # L_out < 1
    ("L_out", dict(input=_fake((1, 4, 5)), weight=_fake((8, 4, 9)), padding=1)),
    ("add", dict(add=_fake((10, 8)))),                                                     # add without channels_last_out
    ("add", dict(add=_fake((8, 10)), channels_last_out=True)),                             # add of the wrong shape
    ("input", dict(input=_fake((4, 10)))),
    ("weight", dict(weight=_fake((8, 4)))),
    ("weight", dict(weight=_fake((8, 4, 3), bfloat16))),                                   # mixed dtypes
    ("bias", dict(bias=_fake((7,)))),
    ("activation", dict(activation="relu")),
    ("stride", dict(stride=0)),
    ("padding", dict(padding=-1)),
    ("input", dict(input=_fake((1, 4, 10), int32), weight=_fake((8, 4, 3), int32))),
    ("packed_weight", dict(packed_weight=_fake((3, 64, 32)))),                             # float32 takes no packed weight
    ("out", dict(out=_fake((1, 10, 8)))),                                                  # out of the other layout
]


@pytest.mark.parametrize("arg,over", BAD_CONV, ids=[f"{i}-{a}" for i, (a, _) in enumerate(BAD_CONV)])
def test_conv1d_rejects(arg, over):
    kw = dict(input=_fake((1, 4, 10)), weight=_fake((8, 4, 3)), bias=_fake((8,)), stride=1, padding=1)
    kw.update(over)
    with pytest.raises(ValueError, match=arg):
        conv1d(**kw)


def test_pack_weight_rejects():
    with pytest.raises(ValueError, match="weight"):
        conv1d_pack_weight(_fake((8, 4, 3)))                   # float32
    with pytest.raises(ValueError, match="weight"):
        conv1d_pack_weight(_fake((8, 4), bfloat16))


def test_sdpa_noncausal_rejects():
    q, k = _fake((4, 5, 64), bfloat16), _fake((2, 9, 64), bfloat16)
    with pytest.raises(ValueError, match="n_heads"):
        sdpa_noncausal(q, _fake((3, 9, 64), bfloat16), _fake((3, 9, 64), bfloat16))
    with pytest.raises(ValueError, match="head_dim"):
        sdpa_noncausal(q, _fake((2, 9, 32), bfloat16), _fake((2, 9, 32), bfloat16))
    with pytest.raises(ValueError, match="seq_len"):
        sdpa_noncausal(q, k, _fake((2, 8, 64), bfloat16))
    with pytest.raises(ValueError, match="dtype"):
        sdpa_noncausal(q, k, _fake((2, 9, 64), float16))
    with pytest.raises(ValueError, match="out"):
        sdpa_noncausal(q, k, k, out=_fake((4, 9, 64), bfloat16))
    with pytest.raises(ValueError, match="n_heads"):
        sdpa_noncausal_strided(q, k, k, q, 4, 3, 5, 9, 64, (64, 256), (64, 128), (64, 256))
    with pytest.raises(ValueError, match="strides"):
        sdpa_noncausal_strided(q, k, k, q, 4, 2, 5, 9, 64, (64, -256), (64, 128), (64, 256))
