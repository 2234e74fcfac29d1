"""The Whisper decoder and ln_linear without a GPU: the NumPy oracle (tests/whisper_decoder_ref.py) against the reference's
recorded float32 CPU results (tests/golden/g11_whisper_decoder.npz), the cached step against the forward, the proof that the GPU
tests' bars separate right from wrong, the exported surface, the C ABI of the new entry points, the loader, the host-only plan
and the argument checks (which run before anything touches a device)."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from pygpukit_amd import _hip
from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import bfloat16, float16, float32, int32
from pygpukit_amd.ops.nn.linear import (LN_LINEAR_K_SPECIALIZATIONS, embed_token_position_ptr, ln_linear, ln_linear_plan,
                                       ln_linear_qkv_cache_ptr)
from tests import whisper_decoder_ref as R
from tests.conftest import load_golden, rel_err
from tests.test_whisper_cpu import _ctype_of, _header_prototypes

g11 = load_golden("g11_whisper_decoder.npz")
NEW_ENTRIES = ("pgk_ln_linear", "pgk_ln_linear_plan", "pgk_ln_linear_qkv_cache", "pgk_embed_token_position")


@pytest.fixture(scope="module")
def fx():
    cfg = R.fixture_config()
    tensors = R.make_decoder_weights(cfg, int(g11["seed"]))
    return cfg, tensors, g11["enc"][0]


# ---- 1. oracle against the fixture ------------------------------------------------------------------------------------------
def test_oracle_matches_the_reference_logits(fx):
    """rel_err(fixture, ref64) = 3.7e-7 and rel_err(ref32, fixture) = 3.8e-7 as measured: float32 in another summation order.
    The bar is a few float32 ulps of logits of magnitude <= 4."""
    cfg, tensors, enc = fx
    assert int(g11["seed"]) == R.FIXTURE_SEED and tuple(g11["ids"][0]) == R.FIXTURE_IDS and g11["enc"].shape == (1, 37, 128)
    want = g11["logits"][0]
    assert want.shape == (5, 203) and want.dtype == np.float32
    ref64 = R.DecoderRef(cfg, tensors).forward(R.FIXTURE_IDS, enc)
    ref32 = R.DecoderRef(cfg, tensors, np.float32).forward(R.FIXTURE_IDS, enc)
    assert ref32.dtype == np.float32
    print("rel_err(fixture, ref64) =", rel_err(want, ref64), " rel_err(ref32, fixture) =", rel_err(ref32, want))
    assert rel_err(ref32, want) <= 2e-6
    assert rel_err(want, ref64) <= 2e-6


def test_oracle_greedy_tokens_equal_the_fixture(fx):
    cfg, tensors, enc = fx
    want = [int(t) for t in g11["tokens"]]
    assert len(want) == R.FIXTURE_STEPS and want[0] == cfg.decoder_start_token_id and cfg.eos_token_id not in want
    for dtype in (np.float64, np.float32):
        for use_cache in (True, False):
            assert R.DecoderRef(cfg, tensors, dtype).generate(enc, R.FIXTURE_STEPS, use_cache=use_cache) == want


def test_oracle_meets_the_16_bit_generation_condition(fx):
    """tests/test_whisper_decoder_gpu.py compares 16-bit tokens up to the first step whose oracle gap is below 4x the measured
    logit error and needs 8 steps: on rounded weights the first 10 gaps are all >= 3e-2 of the largest |logit| (0.1 absolute)."""
    cfg, tensors, enc = fx
    for rd in ("bf16", "f16"):
        _, rows = R.DecoderRef(cfg, tensors, np.float64, rd).generate(enc, R.FIXTURE_STEPS, return_logits=True)
        gaps = np.array([R.top2_gap(r) for r in rows[:10]])
        assert gaps.min() >= 3e-2 * np.abs(rows).max() and gaps.min() >= 0.1, (rd, gaps)


# ---- 2. cached step against forward -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("round_dtype", ["f32", "bf16"])
def test_cached_step_equals_forward_at_every_position(fx, round_dtype):
    cfg, tensors, enc = fx
    tokens = [int(t) for t in g11["tokens"]] + [5, 9, 11, 13]                      # 24 tokens: the whole position table
    assert len(tokens) == cfg.max_target_positions
    ref = R.DecoderRef(cfg, tensors, np.float64, round_dtype)
    full = ref.forward(tokens, enc)
    ref.set_encoder_states(enc)
    for pos, t in enumerate(tokens):
        assert np.max(np.abs(ref.step(t, pos) - full[pos])) <= 1e-12, pos


# ---- 3. mutations ---------------------------------------------------------------------------------------------------------------
WIDEST_GPU_BAR = 2e-2        # tests/test_whisper_decoder_gpu.py: rel_err 1e-2 per position in 16 bits, twice that step against forward


def _per_position(fx, mutation):
    cfg, tensors, enc = fx
    tokens = [int(t) for t in g11["tokens"]]
    right, wrong = R.DecoderRef(cfg, tensors), R.DecoderRef(cfg, tensors, mutate=mutation)
    right.set_encoder_states(enc)
    wrong.set_encoder_states(enc)
    step = [rel_err(wrong.step(t, p), right.step(t, p)) for p, t in enumerate(tokens)]
    good = right.forward(tokens, enc)
    fwd = [rel_err(w, g) for w, g in zip(wrong.forward(tokens, enc), good)]
    return np.array(step), np.array(fwd)


@pytest.mark.parametrize("mutation", [m for m in R.MUTATIONS if m not in ("drop_k_bias_zero", "v_bias_on_q")])
def test_every_planted_error_moves_the_logits_far_beyond_the_widest_bar(fx, mutation):
    """The GPU tests assert their bar at EVERY position, so a planted error is caught where it moves the logits most: that
    movement is at least 25x the widest bar.  Measured (largest / smallest per-position rel_err): cross_is_causal 0.69 / 0.20,
    position_off_by_one 1.06 / 0.79, skip_final_norm 1.23 / 0.76, stale_cache_row (cached step only; position 0 is untouched)
    0.55 / 0.37 from position 1 on."""
    step, fwd = _per_position(fx, mutation)
    print(mutation, "step", step.max(), step.min(), "forward", fwd.max(), fwd.min())
    assert step.max() >= 25 * WIDEST_GPU_BAR, (mutation, step)
    if mutation == "stale_cache_row":
        assert step[0] == 0.0 and fwd.max() == 0.0 and step[1:].min() >= 15 * WIDEST_GPU_BAR
    else:
        assert np.allclose(step, fwd, rtol=1e-9) and fwd.min() >= 10 * WIDEST_GPU_BAR


def test_a_bias_on_k_cannot_be_seen_and_that_is_why_zeros_are_right(fx):
    """drop_k_bias_zero (v_proj's bias used for k) moves NOTHING: a bias on every key adds q . b to every score of a row, and
    softmax is invariant under a row-constant shift - the reason Whisper's k_proj has no bias.  No bar can catch it, so it
    is the one planted error checked for invariance instead of movement: what the decoder does with the absent bias (zeros) is
    as right as any other choice."""
    step, fwd = _per_position(fx, "drop_k_bias_zero")
    assert step.max() <= 1e-12 and fwd.max() <= 1e-12


def test_a_bias_in_the_wrong_slot_is_seen_by_the_float32_bar(fx):
    """The bias error that CAN be seen, in place of the one that cannot: v_proj's bias added to q (the order of a fused q | k | v
    bias vector mixed up).  The fixture's biases have scale 0.1, so it moves the logits by 0.024 .. 0.077 per position: at least
    100x the float32 bars (never above 1e-4, doubled for step against forward) at EVERY position, but only 1.2x .. 3.8x the
    16-bit bar of 2e-2 - it is the float32 GPU tests that catch an error of this size."""
    step, fwd = _per_position(fx, "v_bias_on_q")
    assert np.allclose(step, fwd, rtol=1e-9)
    assert fwd.min() >= 100 * 2e-4 and fwd.min() >= WIDEST_GPU_BAR and fwd.max() >= 3 * WIDEST_GPU_BAR


def test_unknown_mutation_is_rejected(fx):
    cfg, tensors, _ = fx
    with pytest.raises(ValueError):
        R.DecoderRef(cfg, tensors, mutate="swap")


# ---- ln_linear: the float32 restatement stays inside the derived bar --------------------------------------------------------------
@pytest.mark.parametrize("round_dtype", ["f32", "bf16", "f16"])
def test_float32_restatement_stays_inside_the_ln_linear_bar(round_dtype):
    """n_ln = 2K + 8 holds: worst |err| / bar of the float32 NumPy restatement over every shape and variant is 0.041 (float32),
    0.979 (bf16) and 0.948 (f16) - in the 16-bit types almost all of it is the output rounding itself."""
    worst = 0.0
    for shape in R.LN_SHAPES:
        for variant in R.LN_VARIANTS:
            c = R.make_ln_case(shape, variant, round_dtype)
            got = R.round_to(R.ln_linear(c, np.float32), round_dtype).astype(np.float64)
            worst = max(worst, float(np.max(np.abs(got - R.ln_linear(c)) / R.ln_bar(c, round_dtype))))
    print(round_dtype, "worst ratio", worst)
    assert worst <= 1.0


def test_ln_linear_bar_separates_a_dropped_beta_and_a_sample_variance():
    """Two errors a fused kernel can make: forgetting beta (moves x^ by 0.1) and the sample variance K / (K - 1) (x^ - beta
    scaled by sqrt((K - 1) / K), restated here through gamma)."""
    for rd, least in (("f32", 25.0), ("bf16", 25.0)):
        c = R.make_ln_case((1, 128, 203), "ln", rd)
        right, bar = R.ln_linear(c), R.ln_bar(c, rd)
        no_beta = R.ln_linear({**c, "beta": np.zeros_like(c["beta"])})
        assert np.max(np.abs(no_beta - right) / bar) >= least
    c = R.make_ln_case((1, 128, 203), "ln", "f32")
    k = c["x"].shape[1]
    sample = R.ln_linear({**c, "gamma": np.asarray(c["gamma"], np.float64) * np.sqrt((k - 1) / k)})
    assert np.max(np.abs(sample - R.ln_linear(c)) / R.ln_bar(c, "f32")) >= 25


# ---- 4. surface -------------------------------------------------------------------------------------------------------------------
def test_names_importable_where_the_reference_has_them():
    import pygpukit_amd
    from pygpukit_amd import asr, ops
    from pygpukit_amd.asr import whisper
    from pygpukit_amd.ops import basic, nn

    for name, fn in (("ln_linear", ln_linear), ("ln_linear_plan", ln_linear_plan), ("ln_linear_qkv_cache_ptr", ln_linear_qkv_cache_ptr),
                     ("embed_token_position_ptr", embed_token_position_ptr)):
        for mod in (nn, ops, basic, pygpukit_amd):
            assert getattr(mod, name) is fn, (mod.__name__, name)
        assert name in nn.__all__ and name in ops.__all__ and name in basic.__all__
    assert len(set(nn.__all__)) == len(nn.__all__)
    for name in ("WhisperDecoder", "WhisperDecoderLayer", "create_decoder"):
        assert getattr(whisper, name) is getattr(asr, name) and name in whisper.__all__ and name in asr.__all__
    assert len(set(whisper.__all__)) == len(whisper.__all__)


# ---- 5. C ABI -----------------------------------------------------------------------------------------------------------------------
def test_header_prototypes_and_exports_agree_for_the_new_entries():
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


# ---- 6. loader ------------------------------------------------------------------------------------------------------------------------
def test_loader_fills_the_decoder_side(fx):
    from pygpukit_amd.asr.whisper import WhisperWeights, create_decoder
    from tests import whisper_ref as E

    cfg, tensors, _ = fx
    w = WhisperWeights.from_tensors(cfg, tensors)
    assert w.decoder_embed_tokens.shape == (203, 128) and w.decoder_embed_positions.shape == (24, 128)
    assert w.decoder_layer_norm_weight.shape == (128,) and w.decoder_layer_norm_bias.shape == (128,)
    assert w.proj_out_weight.shape == (203, 128) and w.proj_out_weight is not w.decoder_embed_tokens
    assert len(w.decoder_layers) == 2 and w.encoder_layers == [] and w.encoder_conv1_weight is None
    layer = w.decoder_layers[1]
    assert len(layer) == 26 and layer["self_attn_k_bias"] is None and layer["cross_attn_k_bias"] is None
    assert layer["cross_attn_q_weight"] is not None and np.array_equal(
        layer["cross_attn_q_weight"], tensors["model.decoder.layers.1.encoder_attn.q_proj.weight"])
    assert layer["fc1_weight"].shape == (256, 128) and layer["cross_attn_layer_norm_bias"].shape == (128,)
    expected = {f"{a}_attn_{p}_{k}" for a in ("self", "cross") for p in ("q", "k", "v", "out") for k in ("weight", "bias")}
    expected |= {f"{a}_attn_layer_norm_{k}" for a in ("self", "cross") for k in ("weight", "bias")}
    expected |= {f"{n}_{k}" for n in ("fc1", "fc2", "final_layer_norm") for k in ("weight", "bias")}
    assert set(layer) == expected
    # k_proj biases are taken when present
    with_k = {**tensors, "model.decoder.layers.0.self_attn.k_proj.bias": np.ones(128, np.float32)}
    assert WhisperWeights.from_tensors(cfg, with_k).decoder_layers[0]["self_attn_k_bias"].shape == (128,)
    # tied output projection
    tied = {k: v for k, v in tensors.items() if k != "proj_out.weight"}
    wt = WhisperWeights.from_tensors(cfg, tied)
    assert wt.proj_out_weight is wt.decoder_embed_tokens
    # a missing tensor is named
    for gone in ("model.decoder.layers.1.encoder_attn.v_proj.bias", "model.decoder.layer_norm.weight", "model.decoder.embed_positions.weight"):
        with pytest.raises(KeyError, match=gone.rsplit(".", 2)[-2]):
            WhisperWeights.from_tensors(cfg, {k: v for k, v in tensors.items() if k != gone})
    # any encoder tensor present: the whole encoder is required (a truncated checkpoint still raises)
    with pytest.raises(KeyError, match="conv1.weight"):
        WhisperWeights.from_tensors(cfg, {**tensors, "model.encoder.layer_norm.bias": np.zeros(128, np.float32)})
    # encoder and decoder together; encoder-only dicts load as before and cannot make a decoder
    both = WhisperWeights.from_tensors(cfg, {**E.make_weights(cfg, 3), **tensors})
    assert len(both.encoder_layers) == 2 and len(both.decoder_layers) == 2
    enc_only = WhisperWeights.from_tensors(cfg, E.make_weights(cfg, 3))
    assert enc_only.decoder_embed_tokens is None and enc_only.decoder_layers == [] and enc_only.proj_out_weight is None
    assert len(enc_only.encoder_layers) == 2
    with pytest.raises(ValueError, match="decoder"):
        create_decoder(cfg, enc_only)


# ---- 7. host-only plan and arguments ------------------------------------------------------------------------------------------------------
def test_plan(monkeypatch):
    monkeypatch.delenv("PGK_LN_LINEAR_GENERIC", raising=False)
    assert LN_LINEAR_K_SPECIALIZATIONS == ()                               # K is a runtime argument on every path
    for dt in (float32, bfloat16, float16, "bfloat16"):
        assert ln_linear_plan(1, 1280, 5120, dt) == "fp32_image"
        assert ln_linear_plan(1, 5120, 1280, dt, norm=False) == "fp32_image"
        assert ln_linear_plan(1, 128, 203, dt) == "fp32_image"
        assert ln_linear_plan(3, 204, 37, dt) == "generic" and ln_linear_plan(3, 200, 37, dt) == "fp32_image" and ln_linear_plan(1, 1284, 8, dt) == "generic"      # K % 8 != 0
        assert ln_linear_plan(1, 128, 203, dt, aligned=False) == "generic"                                       # misaligned pointers
        assert ln_linear_plan(8, 2048, 24, dt) == "fp32_image" and ln_linear_plan(8, 2056, 24, dt) == "generic"  # 64 KB exactly / beyond
        assert ln_linear_plan(8, 5120, 16, dt, norm=False) == "generic"                                          # 80 KB even in 16 bits
    for dt in (bfloat16, float16):
        assert ln_linear_plan(4, 5120, 24, dt, norm=False) == "dtype_image" and ln_linear_plan(4, 5120, 24, dt) == "generic"
        assert ln_linear_plan(8, 4096, 24, dt, norm=False) == "dtype_image" and ln_linear_plan(8, 4104, 24, dt, norm=False) == "generic"
    assert ln_linear_plan(4, 5120, 24, float32, norm=False) == "generic"
    monkeypatch.setenv("PGK_LN_LINEAR_GENERIC", "1")
    assert ln_linear_plan(1, 1280, 5120, bfloat16) == "generic"
    monkeypatch.setenv("PGK_LN_LINEAR_GENERIC", "0")
    assert ln_linear_plan(1, 1280, 5120, bfloat16) == "fp32_image"


@pytest.mark.parametrize("args", [(0, 128, 8), (9, 128, 8), (1, 0, 8), (1, 128, 0)], ids=str)
def test_plan_rejects_bad_shapes(args):
    with pytest.raises(ValueError):
        ln_linear_plan(*args, bfloat16)
    with pytest.raises(ValueError):
        ln_linear_plan(1, 128, 8, int32)


def test_decode_launches_formula(monkeypatch):
    """DESIGN.md section 4.4 states 10 per layer + 3 fused and 19 per layer + 6 unfused.  This only re-evaluates the method's
    arithmetic on the host, with the attention op's switch in both positions; what pins the count to the kernels that really run
    is the graph-node assertion of tests/test_whisper_decoder_gpu.py."""
    from pygpukit_amd.asr.whisper import WhisperDecoder

    for switch, cross in ((None, 2), ("auto", 2), ("1", 2), ("0", 1), ("off", 1)):
        if switch is None:
            monkeypatch.delenv("PYGPUKIT_FLASH_DECODING", raising=False)
        else:
            monkeypatch.setenv("PYGPUKIT_FLASH_DECODING", switch)
        for layers in (2, 32):
            for fused, want in ((True, (8 + cross) * layers + 3), (False, (17 + cross) * layers + 6)):
                d = WhisperDecoder.__new__(WhisperDecoder)
                d.n_layers, d.fused = layers, fused
                assert d.decode_launches() == want


def _fake(shape, dtype=float32, ptr=0x1000):
    return GPUArray(shape, dtype, device_ptr=ptr, owns_memory=False)       # never dereferenced: the checks come first


def test_ln_linear_rejects():
    x, w = _fake((1, 128)), _fake((24, 128), ptr=0x10000)
    g = _fake((128,), ptr=0x20000)
    with pytest.raises(ValueError, match="alias"):
        ln_linear(x, _fake((128, 128), ptr=0x10000), out=x)
    with pytest.raises(ValueError, match="beta without gamma"):
        ln_linear(x, w, beta=g)
    with pytest.raises(ValueError, match="gamma"):
        ln_linear(x, w, gamma=g)
    with pytest.raises(ValueError, match="rows"):
        ln_linear(_fake((9, 128)), w)
    with pytest.raises(ValueError, match="mismatch"):
        ln_linear(_fake((1, 64)), w)
    with pytest.raises(ValueError, match="bias"):
        ln_linear(x, w, _fake((23,)))
    with pytest.raises(ValueError, match="weight"):
        ln_linear(x, _fake((24, 128), bfloat16))
    with pytest.raises(ValueError, match="activation"):
        ln_linear(x, w, activation="relu")
    with pytest.raises(ValueError, match="residual"):
        ln_linear(x, w, residual=_fake((1, 23)))
    with pytest.raises(ValueError, match="out"):
        ln_linear(x, w, out=_fake((1, 23)))
    with pytest.raises(ValueError):
        ln_linear(_fake((1, 128), int32), _fake((24, 128), int32))


def test_ln_linear_qkv_cache_and_embed_reject():
    x, w, b = _fake((1, 128)), _fake((384, 128), ptr=0x10000), _fake((384,), ptr=0x40000)
    q, kc, vc = _fake((1, 128), ptr=0x50000), _fake((2, 24, 64), ptr=0x60000), _fake((2, 24, 64), ptr=0x70000)
    pos = _fake((1,), int32, ptr=0x80000)
    for position in (24, -1):                                              # outside the cache
        with pytest.raises(ValueError, match="position"):
            ln_linear_qkv_cache_ptr(x, w, b, q, kc, vc, position=position)
    with pytest.raises(ValueError, match="position"):
        ln_linear_qkv_cache_ptr(x, w, b, q, kc, vc)                        # neither
    with pytest.raises(ValueError, match="position"):
        ln_linear_qkv_cache_ptr(x, w, b, q, kc, vc, pos, position=3)       # both
    with pytest.raises(ValueError, match="int32"):
        ln_linear_qkv_cache_ptr(x, w, b, q, kc, vc, _fake((1,), float32))
    with pytest.raises(ValueError, match="caches"):
        ln_linear_qkv_cache_ptr(x, w, b, q, kc, _fake((2, 25, 64)), pos)
    with pytest.raises(ValueError, match="qkv_weight"):
        ln_linear_qkv_cache_ptr(x, _fake((256, 128)), None, q, kc, vc, pos)
    with pytest.raises(ValueError, match="q_out"):
        ln_linear_qkv_cache_ptr(x, w, b, _fake((1, 64)), kc, vc, pos)
    tok, pt, out, st = _fake((203, 128)), _fake((24, 128)), _fake((1, 128)), _fake((3,), int32)
    with pytest.raises(ValueError, match="tables"):
        embed_token_position_ptr(tok, _fake((24, 64)), out, st)
    with pytest.raises(ValueError, match="out"):
        embed_token_position_ptr(tok, pt, _fake((1, 64)), st)
    with pytest.raises(ValueError, match="state_buf"):
        embed_token_position_ptr(tok, pt, out, _fake((1,), int32))
    with pytest.raises(ValueError, match="state_buf"):
        embed_token_position_ptr(tok, pt, out, _fake((3,), float32))


def test_library_argument_errors_return_invalid_without_a_device():
    """The C entry points check their arguments before resolving a stream or launching: PGK_ERR_INVALID with no GPU present."""
    lib = _hip.load()
    p = lambda v: C.c_void_p(v)                                             # noqa: E731
    f32 = float32.code
    ok = dict(x=p(0x1000), gamma=None, beta=None, w=p(0x10000), bias=None, residual=None, out=p(0x90000))

    def run(m=1, k=128, n=24, act=0, dt=f32, **over):
        a = {**ok, **over}
        return lib.pgk_ln_linear(a["x"], a["gamma"], a["beta"], a["w"], a["bias"], a["residual"], a["out"], m, k, n, C.c_float(1e-5), act, dt, None)

    invalid = 1
    assert run(out=p(0x1000)) == invalid and b"alias" in lib.pgk_last_error()            # x aliasing out
    assert run(out=p(0x1000 + 64)) == invalid                                             # overlapping, not equal
    assert run(beta=p(0x20000)) == invalid and b"beta" in lib.pgk_last_error()            # beta without gamma
    assert run(m=9) == invalid and run(m=0) == invalid
    assert run(act=2) == invalid and run(dt=int32.code) == invalid and run(k=0) == invalid
    q = lib.pgk_ln_linear_qkv_cache
    for h_pos in (24, -1):
        assert q(p(0x1000), None, None, p(0x10000), None, p(0x50000), p(0x60000), p(0x70000), 128, 2, 64, 24, C.c_float(1e-5), h_pos, None,
                 f32, None) == invalid
        assert b"position" in lib.pgk_last_error()
    for k_cache, v_cache in ((0x1000, 0x70000), (0x60000, 0x1000 + 128)):                 # x inside a cache: rows stored while x is read
        assert q(p(0x1000), None, None, p(0x10000), None, p(0x50000), p(k_cache), p(v_cache), 128, 2, 64, 24, C.c_float(1e-5), 0, None,
                 f32, None) == invalid
        assert b"cache" in lib.pgk_last_error()
    assert lib.pgk_embed_token_position(p(0x1000), p(0x2000), p(0x3000), 128, 203, 24, None, f32, None) == invalid
