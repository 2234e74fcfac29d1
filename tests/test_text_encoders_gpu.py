"""T5Encoder, CLIPTextEncoder and FluxPipeline with both, on the GPU, on the configurations of tests/golden/g16_text_encoders.npz,
against HuggingFace transformers' recorded float64 outputs, the reference's recorded float32 CPU output and the float64
restatements of tests/t5_ref.py / tests/clip_ref.py.

Bars.  float32: t5_ref.f32_bar - 8 times the float32 restatement's own distance from the float64 one on these inputs, at most 1e-4
(derivation in tests/t5_ref.py).  bfloat16: rel_err <= 1e-2 against the float64 restatement on weights rounded to bfloat16, the
project's 16-bit bar.  The masked element is compared on its valid rows and on all rows (both programs compute the padded query
rows too).

Measured on an MI355X.  T5 float32: 3.83e-7 (HF mode) and 3.16e-7 (reference mode) against bars of 3.08e-6 and 2.48e-6; T5 bfloat16:
5.63e-3 and 5.40e-3.  CLIP float32: hidden 5.90e-7, pooled 6.68e-7 against a bar of 4.73e-6.  CLIP bfloat16: hidden 5.54e-3,
pooled 6.38e-3 with the float32 residual stream CLIPTextEncoder keeps (with a bfloat16 stream, rounded after every add, they were
7.72e-3 and 1.083e-2 - the pooled rows above the bar; the fixture's q / k projections give attention logits of standard deviation
4, at which the rounding of q and k alone moves a probability by about half a percent)."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from oracle import cpu_ref as O
from tests import clip_ref as C
from tests import t5_ref as T
from tests.conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

g16 = load_golden("g16_text_encoders.npz")
T5_CFG, CLIP_CFG = T.fixture_config(), C.fixture_config()
NAMES = {"f32": "float32", "bf16": "bfloat16"}


def _round_bf16(a):
    return O.bf16_bits_to_f32(O.f32_to_bf16_bits(np.ascontiguousarray(a, np.float32)))


def _host(a) -> np.ndarray:
    from pygpukit_amd.core.dtypes import float32

    return a.astype(float32).to_numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def _t5_weights():
    return T.make_weights(T5_CFG, int(g16["t5_seed"]))


@functools.lru_cache(maxsize=None)
def _clip_weights():
    return C.make_weights(CLIP_CFG, int(g16["clip_seed"]))


@functools.lru_cache(maxsize=None)
def _t5(dtype, mode="hf"):
    from pygpukit_amd.diffusion import T5Encoder

    kw = {} if mode == "hf" else dict(attention_scale=None, ffn_activation="relu")
    return T5Encoder(hidden_size=T5_CFG["d_model"], num_layers=T5_CFG["num_layers"], num_heads=T5_CFG["num_heads"], d_ff=T5_CFG["d_ff"],
                     max_length=T5_CFG["seq"], weights=_t5_weights(), dtype=NAMES[dtype], **kw)


@functools.lru_cache(maxsize=None)
def _clip(dtype):
    from pygpukit_amd.diffusion import CLIPTextEncoder

    return CLIPTextEncoder(hidden_size=CLIP_CFG["hidden_size"], num_layers=CLIP_CFG["num_layers"], num_heads=CLIP_CFG["num_heads"],
                           max_length=CLIP_CFG["seq"], weights=_clip_weights(), dtype=NAMES[dtype], hidden_act=CLIP_CFG["hidden_act"],
                           eos_token_id=CLIP_CFG["eos_token_id"])


@functools.lru_cache(maxsize=None)
def _t5_ref(mode, dtype="f64", rounded=False):
    ids, mask = g16["t5_ids"].astype(np.int64), g16["t5_mask"].astype(np.int64)
    return T.t5_forward(T5_CFG, _t5_weights(), ids, mask, mode, np.float64 if dtype == "f64" else np.float32, _round_bf16 if rounded else None)


@functools.lru_cache(maxsize=None)
def _clip_ref(dtype="f64", rounded=False):
    return C.clip_forward(CLIP_CFG, _clip_weights(), g16["clip_ids"].astype(np.int64), np.float64 if dtype == "f64" else np.float32,
                          _round_bf16 if rounded else None)


def _t5_bar(dtype, mode):
    return T.BAR16 if dtype == "bf16" else T.f32_bar(_t5_ref(mode, "f32"), _t5_ref(mode))


@pytest.mark.parametrize("mode,key", [("hf", "t5_hf_out"), ("reference", "t5_ref_out")])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_t5_matches_the_fixture(dtype, mode, key):
    enc = _t5(dtype, mode)
    assert enc.inner == 192 != enc.hidden_size and enc.d_kv == 64
    assert enc.plan(T5_CFG["seq"])["attention"] == ("relbias_rows" if dtype == "f32" else "relbias_flash")
    got = _host(enc.forward(g16["t5_ids"], g16["t5_mask"]))
    ref = _t5_ref(mode, rounded=dtype == "bf16")
    bar = _t5_bar(dtype, mode)
    e, e_fix = rel_err(got, ref), rel_err(got, g16[key])
    n1 = T5_CFG["valid"][1]
    e_valid = rel_err(got[1, :n1], ref[1, :n1])
    print(f"T5 {mode} {dtype}: rel_err vs the float64 restatement {e:.3e} (valid rows of the masked element {e_valid:.3e}), vs the recorded "
          f"fixture {e_fix:.3e}, bar {bar:.3e}")
    assert got.shape == (2, T5_CFG["seq"], T5_CFG["d_model"]) and np.isfinite(got).all()
    assert e <= bar and e_valid <= bar
    if dtype == "f32":      # the fixture itself is float32 arithmetic (the reference) or carries a float32 softmax (HF): twice the bar
        assert e_fix <= 2 * bar
    # the other mode's oracle is far: the scale and the gate are really switched
    other = _t5_ref("reference" if mode == "hf" else "hf")
    assert rel_err(got, other) > 0.05


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_t5_mask_keeps_the_padded_tail_out_of_the_valid_rows(dtype):
    enc = _t5(dtype)
    ids, mask = g16["t5_ids"].astype(np.int64), g16["t5_mask"]
    n1 = T5_CFG["valid"][1]
    base = enc.forward(ids, mask).to_numpy()
    changed = ids.copy()
    changed[1, n1:] = (changed[1, n1:] + 7) % T5_CFG["vocab_size"]
    again = enc.forward(changed, mask).to_numpy()
    assert np.array_equal(base[0], again[0]) and np.array_equal(base[1, :n1], again[1, :n1])
    assert not np.array_equal(base[1, n1:], again[1, n1:])
    unmasked = _host(enc.forward(ids, None))
    assert rel_err(unmasked[1, :n1], _t5_ref("hf")[1, :n1]) > 5 * T.BAR16          # without the mask the valid rows attend the tail
    with pytest.raises(ValueError, match="prefix mask"):
        hole = np.asarray(mask).copy()
        hole[0, 5] = 0
        enc.forward(ids, hole)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_clip_matches_the_fixture(dtype):
    enc = _clip(dtype)
    hidden, pooled = enc.forward(g16["clip_ids"], g16["clip_mask"])
    hidden, pooled = _host(hidden), _host(pooled)
    ref_h, ref_p = _clip_ref(rounded=dtype == "bf16")
    ref32_h, _ = _clip_ref("f32")
    bar = T.BAR16 if dtype == "bf16" else T.f32_bar(ref32_h, _clip_ref()[0])
    eh, ep = rel_err(hidden, ref_h), rel_err(pooled, ref_p)
    print(f"CLIP {dtype}: hidden rel_err {eh:.3e}, pooled {ep:.3e} vs the float64 restatement; vs the fixture {rel_err(hidden, g16['clip_hidden']):.3e}, "
          f"{rel_err(pooled, g16['clip_pooled']):.3e}; bar {bar:.3e}")
    assert hidden.shape == (2, 77, CLIP_CFG["hidden_size"]) and pooled.shape == (2, CLIP_CFG["hidden_size"])
    assert eh <= bar and ep <= bar
    if dtype == "f32":
        assert rel_err(hidden, g16["clip_hidden"]) <= 2 * bar and rel_err(pooled, g16["clip_pooled"]) <= 2 * bar
    for b, at in enumerate(CLIP_CFG["eos_at"]):      # the pooled row is the hidden row at the EOS, not the last row
        assert np.array_equal(pooled[b], hidden[b, at])
    assert rel_err(pooled[0], ref_h[0, -1]) > 0.05


def test_clip_pooled_is_independent_of_ids_after_the_eos():
    enc = _clip("bf16")
    ids = g16["clip_ids"].astype(np.int64)
    at = CLIP_CFG["eos_at"][0]
    _, base = enc.forward(ids)
    changed = ids.copy()
    changed[0, at + 1:] = 5
    hidden, again = enc.forward(changed)
    assert np.array_equal(base.to_numpy(), again.to_numpy())


def test_clip_text_projection_and_prefixless_names():
    from pygpukit_amd.diffusion import CLIPTextEncoder

    w = {n[len(C.PREFIX):]: a for n, a in _clip_weights().items()}
    proj = (np.random.default_rng(3).standard_normal((12, CLIP_CFG["hidden_size"])) / 8).astype(np.float32)
    w["text_projection.weight"] = proj
    enc = CLIPTextEncoder(hidden_size=CLIP_CFG["hidden_size"], num_layers=CLIP_CFG["num_layers"], num_heads=CLIP_CFG["num_heads"],
                          max_length=77, weights=w, dtype="float32", eos_token_id=CLIP_CFG["eos_token_id"])
    _, pooled = enc.forward(g16["clip_ids"])
    ref = _clip_ref()[1] @ proj.astype(np.float64).T
    assert pooled.shape == (2, 12) and rel_err(_host(pooled), ref) <= 1e-4


def test_encode_runs_end_to_end_without_files():
    from pygpukit_amd.diffusion import CLIPTextEncoder, T5Encoder

    rng = np.random.default_rng(0)
    tw = dict(_t5_weights())
    tw["shared.weight"] = rng.standard_normal((200, T5_CFG["d_model"])).astype(np.float32)     # 'a cat' needs ids up to 116
    t5 = T5Encoder(hidden_size=T5_CFG["d_model"], num_layers=T5_CFG["num_layers"], num_heads=T5_CFG["num_heads"], d_ff=T5_CFG["d_ff"],
                   max_length=24, weights=tw, dtype="bfloat16")
    out = t5.encode("a cat")
    assert out.shape == (1, 24, T5_CFG["d_model"]) and np.isfinite(_host(out)).all()
    cw = dict(_clip_weights())
    cw[C.PREFIX + "embeddings.token_embedding.weight"] = rng.standard_normal((49408, CLIP_CFG["hidden_size"])).astype(np.float32)
    clip = CLIPTextEncoder(hidden_size=CLIP_CFG["hidden_size"], num_layers=CLIP_CFG["num_layers"], num_heads=CLIP_CFG["num_heads"], weights=cw,
                           dtype="bfloat16")
    hidden, pooled = clip.encode(["a cat", "a dog on a mat"])
    assert hidden.shape == (2, 77, CLIP_CFG["hidden_size"]) and pooled.shape == (2, CLIP_CFG["hidden_size"])
    assert np.array_equal(_host(pooled)[0], _host(hidden)[0, 6])       # BOS + 5 characters, then the EOS


def test_flux_pipeline_takes_a_prompt():
    """FluxPipeline(text_encoder=, text_encoder_2=)(prompt=...) equals the call with the same embeddings passed explicitly."""
    from pygpukit_amd.diffusion import VAE, CLIPTextEncoder, FluxPipeline, FluxTransformer, T5Encoder
    from pygpukit_amd.diffusion import FluxConfig, VAESpec
    from tests import flux_ref as R
    from tests import vae_ref as V

    cfg = R.fixture_config()
    pk_cfg = FluxConfig(in_channels=cfg.in_channels, hidden_size=cfg.hidden_size, num_layers=cfg.num_layers,
                        num_single_layers=cfg.num_single_layers, num_attention_heads=cfg.num_attention_heads,
                        attention_head_dim=cfg.attention_head_dim, joint_attention_dim=cfg.joint_attention_dim,
                        pooled_projection_dim=cfg.pooled_projection_dim, guidance_embeds=cfg.guidance_embeds, axes_dims_rope=cfg.axes_dims_rope)
    vae_spec = VAESpec(name="flux_fixture_vae", latent_channels=2, scaling_factor=0.5, block_out_channels=(8, 16, 16, 16), layers_per_block=1,
                       norm_num_groups=4, norm_eps=1e-6, shift_factor=0.25)
    rng = np.random.default_rng(1)
    t5_cfg = dict(T5_CFG, d_model=cfg.joint_attention_dim, vocab_size=200, d_ff=32, num_heads=1)
    t5 = T5Encoder(hidden_size=t5_cfg["d_model"], num_layers=2, num_heads=1, d_ff=32, max_length=512, weights=T.make_weights(t5_cfg, 5),
                   dtype="float32")
    ccfg = dict(CLIP_CFG, hidden_size=64, num_heads=1, intermediate_size=64, vocab_size=49408)
    cw = C.make_weights(ccfg, 6)
    cw["text_projection.weight"] = (rng.standard_normal((cfg.pooled_projection_dim, 64)) / 8).astype(np.float32)
    clip = CLIPTextEncoder(hidden_size=64, num_layers=2, num_heads=1, weights=cw, dtype="float32")
    model = FluxTransformer(pk_cfg, R.make_weights(cfg, int(load_golden("g15_flux.npz")["seed"])), dtype="float32")
    vae = VAE(vae_spec, V.make_weights(vae_spec, V.FIXTURE_SEED), dtype="float32")
    pipe = FluxPipeline(model, vae, text_encoder=clip, text_encoder_2=t5)
    pooled, embeds = pipe.encode_prompt("a cat", max_sequence_length=32)
    assert pooled.shape == (1, cfg.pooled_projection_dim) and embeds.shape == (1, 32, cfg.joint_attention_dim)
    unmasked = pipe.encode_prompt("a cat", max_sequence_length=32, mask_padding=False)[1]
    assert not np.array_equal(unmasked.to_numpy()[0, :6], embeds.to_numpy()[0, :6])
    image = pipe(prompt="a cat", height=32, width=32, num_inference_steps=1, seed=3)
    pooled512, embeds512 = pipe.encode_prompt("a cat")
    explicit = pipe(embeds512, pooled512, height=32, width=32, num_inference_steps=1, seed=3)
    got = image.to_numpy()
    assert got.shape == (1, 3, 32, 32) and np.isfinite(got).all() and np.array_equal(got, explicit.to_numpy())
    positional = pipe("a cat", height=32, width=32, num_inference_steps=1, seed=3)
    assert np.array_equal(got, positional.to_numpy())
