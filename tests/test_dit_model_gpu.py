"""PixArtTransformer on the GPU, on the configuration of tests/golden/g13_pixart.npz (hidden 144, 2 heads of 72, 2 blocks, a 3 x 5
patch grid, 5 text tokens), against the reference's recorded float32 outputs and the float64 oracle of tests/dit_ref.py.

float32: the yardstick is the reference's own distance from exact arithmetic, rel_err(fixture, ref64) = 4.09e-7 (timestep 500 for
both elements) and 3.98e-7 (timesteps 500 and 37) - a property of the reference's float32 CPU path and of the oracle, nothing of
the code under test.  The bar is FACTOR32 times that distance and never more than 1e-4; FACTOR32 is the smallest power of two at
least twice the worst ratio rel_err(gpu, ref64) / rel_err(fixture, ref64) measured on an MI355X: MEASURED below.

bfloat16 / float16: rel_err <= 1e-2, the project's bar, against the oracle running on the inputs and on the weights the device
holds in 16 bits rounded to the dtype (rounding alone moves this fixture by 2.9e-3 in bfloat16 and 3.5e-4 in float16 against the
unrounded truth, which is why the comparison is against the rounded-input oracle)."""

from __future__ import annotations

import dataclasses
import functools

import numpy as np
import pytest

from tests import dit_ref as R
from tests.conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

g13 = load_golden("g13_pixart.npz")
MEASURED = ("rel_err(gpu, ref64): 4.073e-7, ratio 0.995 (timestep 500); 3.942e-7, 0.991 (timesteps 500, 37); 4.025e-7, 1.011 (second "
            "step on cached text K/V); 3.506e-7, 0.881 (head_dim 64) and 4.288e-7, 1.077 (GEGLU), the last two against the fixture's "
            "yardstick 3.980e-7; twice the worst is 2.155, hence FACTOR32 = 4 and a bar of 1.59e-6")
FACTOR32 = 4.0
CAP32 = 1e-4
BAR16 = 1e-2
NAMES = {"f32": "float32", "bf16": "bfloat16", "f16": "float16"}


def _pk_spec(spec: R.Spec):
    from pygpukit_amd.diffusion import PixArtSpec

    return PixArtSpec(name="fixture", hidden_size=spec.hidden_size, num_layers=spec.num_layers, num_heads=spec.num_heads,
                      conditioning_type="cross_attn", text_encoder_dim=spec.text_dim, pos_embed_type="sinusoidal",
                      patch_size=spec.patch_size, in_channels=spec.in_channels, out_channels=spec.out_channels,
                      cross_attention_dim=spec.text_dim)


@functools.lru_cache(maxsize=None)
def _weights(spec: R.Spec = R.fixture_spec()):
    return R.make_weights(spec, int(g13["seed"]))


@functools.lru_cache(maxsize=None)
def _model(dtype, pad_heads="auto", spec: R.Spec = R.fixture_spec()):
    from pygpukit_amd.diffusion import PixArtTransformer

    return PixArtTransformer(_pk_spec(spec), _weights(spec), dtype=NAMES[dtype], pad_heads=pad_heads)


@functools.lru_cache(maxsize=None)
def _ref64(dtype, key="out_t2", swap=False):
    t = float(g13["timestep"]) if key == "out" else g13["timesteps"]
    out = R.forward(R.fixture_spec(), _weights(), g13["latent"], t, g13["text"], np.float64, round_dtype=dtype, swap_conditioning=swap)
    out.setflags(write=False)
    return out


def _dev(a, dtype):
    from pygpukit_amd.core import from_numpy

    return from_numpy(R.to_words(R.round_to(a, dtype), dtype))


def _host(a, dtype):
    return R.from_words(a.to_numpy(), dtype).astype(np.float64)


def _run(model, dtype, latent=None, timestep=None, text="fixture"):
    latent = g13["latent"] if latent is None else latent
    timestep = g13["timesteps"] if timestep is None else timestep
    text = g13["text"] if isinstance(text, str) else text
    out = model.forward(_dev(latent, dtype), timestep, None if text is None else _dev(text, dtype))
    assert out.shape == (latent.shape[0], 8) + latent.shape[2:] and out.dtype.name == NAMES[dtype]
    return _host(out, dtype)


@pytest.mark.parametrize("key", ["out", "out_t2"])
def test_float32_forward_against_the_reference_and_the_oracle(key):
    yard = rel_err(g13[key], _ref64("f32", key))
    bar = FACTOR32 * yard
    assert 1e-7 < yard < 1e-6 and bar <= CAP32
    got = _run(_model("f32"), "f32", timestep=float(g13["timestep"]) if key == "out" else None)
    e = rel_err(got, _ref64("f32", key))
    print(f"PixArt f32 {key}: rel_err(gpu, ref64) {e:.3e}, rel_err(fixture, ref64) {yard:.3e}, ratio {e / yard:.3f}, "
          f"rel_err(gpu, fixture) {rel_err(got, g13[key]):.3e}")
    assert np.isfinite(got).all() and e <= bar


@pytest.mark.parametrize("pad_heads", [True, False])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_16_bit_forward_padded_and_unpadded(dtype, pad_heads):
    from pygpukit_amd.diffusion import dit_plan

    model = _model(dtype, pad_heads)
    plan = dit_plan(model.spec, NAMES[dtype], pad_heads)
    assert plan == model.plan
    assert plan == ({"head_dim": 72, "head_width": 128, "padded": True, "attention": "flash"} if pad_heads else
                    {"head_dim": 72, "head_width": 72, "padded": False, "attention": "fallback"})
    assert model.blocks[0].qkv_w.shape == (3 * 2 * plan["head_width"], 144) and model.blocks[0].out_w.shape == (144, 2 * plan["head_width"])
    got = _run(model, dtype)
    e, e_fix = rel_err(got, _ref64(dtype)), rel_err(got, g13["out_t2"])
    print(f"PixArt {dtype} pad_heads={pad_heads}: rel_err vs the rounded-input oracle {e:.3e}, vs the reference's float32 fixture {e_fix:.3e}")
    assert np.isfinite(got).all() and e <= BAR16


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_swapped_conditioning_misses_the_bar(dtype):
    """Negative control: the oracle of a model that modulates each batch element with the other's conditioning must be rejected
    by the bar the right one passes - the bars see which batch element a modulation vector belongs to."""
    got = _run(_model(dtype), dtype)
    bar = FACTOR32 * rel_err(g13["out_t2"], _ref64("f32")) if dtype == "f32" else BAR16
    wrong = rel_err(got, _ref64(dtype, swap=True))
    print(f"PixArt {dtype}: rel_err against the swapped-conditioning oracle {wrong:.3e}, bar {bar:.3e}")
    assert rel_err(got, _ref64(dtype)) <= bar < wrong and wrong > 0.1


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_cached_encoder_states(dtype):
    """set_encoder_states + forward(latent, timestep) is the three-argument forward bit for bit; a second step at another
    timestep reuses the cache (no new projection) and is right."""
    model = _model(dtype)
    full = _run(model, dtype)
    n = model.encoder_projections
    model.set_encoder_states(_dev(g13["text"], dtype))
    assert model.encoder_projections == n + 1
    np.testing.assert_array_equal(_run(model, dtype, text=None), full)
    other = np.array([37.0, 900.0], np.float32)
    step2 = _run(model, dtype, timestep=other, text=None)
    assert model.encoder_projections == n + 1
    ref = R.forward(R.fixture_spec(), _weights(), g13["latent"], other, g13["text"], np.float64, round_dtype=dtype)
    e = rel_err(step2, ref)
    print(f"PixArt {dtype} second step on cached text K/V: rel_err {e:.3e}")
    assert e <= (FACTOR32 * rel_err(g13["out_t2"], _ref64("f32")) if dtype == "f32" else BAR16) and rel_err(step2, full) > 0.05
    with pytest.raises(ValueError, match="batch"):
        _run(model, dtype, latent=g13["latent"][:1], text=None)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_batch_element_one_alone_equals_row_one_of_the_batch(dtype):
    model = _model(dtype)
    both = _run(model, dtype)
    alone = _run(model, dtype, latent=g13["latent"][1:], timestep=g13["timesteps"][1:], text=g13["text"][1:])
    if dtype == "f32":
        # the GEMMs pick their kernel by the row count (15 rows against 30), so the float32 sums may differ in order: the bar
        # is the float32 yardstick; the 16-bit model rounds between kernels and is held to the 16-bit bar
        bar = FACTOR32 * rel_err(g13["out_t2"], _ref64("f32"))
    else:
        bar = BAR16
    e = rel_err(alone[0], both[1])
    print(f"PixArt {dtype}: element 1 alone against row 1 of the batch: rel_err {e:.3e}")
    assert e <= bar and rel_err(alone[0], _ref64(dtype)[1]) <= bar and rel_err(alone[0], both[0]) > 0.1


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("variant", ["head64", "geglu"])
def test_other_specs_against_the_oracle(variant, dtype):
    """hidden 128 = 2 heads of 64 (the flash kernel without padding in bfloat16), and the GEGLU feed-forward (ff.net.0.proj with
    twice the rows of ff.net.2's columns)."""
    spec = dataclasses.replace(R.fixture_spec(), hidden_size=128, ff_dim=256) if variant == "head64" else \
        dataclasses.replace(R.fixture_spec(), geglu=True, ff_dim=288)
    model = _model(dtype, "auto", spec)
    if variant == "head64":
        assert model.plan == {"head_dim": 64, "head_width": 64, "padded": False, "attention": "flash" if dtype == "bf16" else "fallback"}
    else:
        assert model.blocks[0].geglu and model.blocks[0].ff1_w.shape == (576, 144)
    got = _run(model, dtype)
    ref = R.forward(spec, _weights(spec), g13["latent"], g13["timesteps"], g13["text"], np.float64, round_dtype=dtype)
    e = rel_err(got, ref)
    print(f"PixArt {variant} {dtype}: rel_err {e:.3e}")
    assert e <= (FACTOR32 * rel_err(g13["out_t2"], _ref64("f32")) if dtype == "f32" else BAR16)


def test_from_safetensors_loads_the_same_model(tmp_path):
    """A model directory written with the project's safetensors writer: the spec is read off the tensors (head_dim 72) and the
    forward is the in-memory model's bit for bit."""
    from pygpukit_amd.diffusion import PixArtTransformer
    from pygpukit_amd.llm.safetensors import save_safetensors

    save_safetensors(str(tmp_path / "diffusion_pytorch_model.safetensors"), {k: (v, "F32") for k, v in _weights().items()})
    model = PixArtTransformer.from_safetensors(tmp_path, dtype="float32")
    spec = model.spec
    assert (spec.hidden_size, spec.num_layers, spec.num_heads, spec.get_head_dim()) == (144, 2, 2, 72)
    assert (spec.in_channels, spec.out_channels, spec.patch_size, spec.text_encoder_dim) == (4, 8, 2, 32)
    np.testing.assert_array_equal(_run(model, "f32"), _run(_model("f32"), "f32"))
    with pytest.raises(FileNotFoundError):
        PixArtTransformer.from_safetensors(tmp_path / "empty_dir_that_is_not_there.safetensors")


def test_forward_needs_encoder_states_and_a_patchable_latent():
    from pygpukit_amd.diffusion import PixArtTransformer

    model = PixArtTransformer(_pk_spec(R.fixture_spec()), _weights(), dtype="float32")
    with pytest.raises(RuntimeError, match="encoder states"):
        model.forward(_dev(g13["latent"], "f32"), 500.0)
    with pytest.raises(ValueError, match="multiples"):
        model.forward(_dev(np.zeros((2, 4, 5, 10), np.float32), "f32"), 500.0, _dev(g13["text"], "f32"))
    with pytest.raises(KeyError, match="proj_out.weight"):
        PixArtTransformer(_pk_spec(R.fixture_spec()), {k: v for k, v in _weights().items() if k != "proj_out.weight"})
