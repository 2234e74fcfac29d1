"""FluxTransformer and FluxPipeline on the GPU, on the configuration of tests/golden/g15_flux.npz (hidden 128, 2 heads of 64, RoPE
axes (16, 24, 24), 2 double + 2 single blocks, 5 text tokens, a 2 x 3 image grid, B = 2), against the reference's recorded float32
outputs and the float64 oracle of tests/flux_ref.py.

float32: the yardstick is the reference's own distance from exact arithmetic, rel_err(fixture, ref64) = 3.39e-7 (one timestep),
3.57e-7 (a timestep per element), 3.20e-7 (guidance) - a property of the reference's float32 CPU path and of the oracle, nothing
of the code under test.  The bar is FACTOR32 times that distance and never more than 1e-4; FACTOR32 is the smallest power of two
at least twice the worst ratio rel_err(gpu, ref64) / rel_err(fixture, ref64) measured on an MI355X: MEASURED below.

bfloat16 / float16: rel_err <= 1e-2, the project's bar, against the oracle on the inputs and weights rounded to the dtype.
tests/test_flux_cpu.py shows that a device which rounds where this one does and is otherwise exact uses less than half of it.

The pipeline (float32): transformer steps, Euler updates, unpack and VAE.decode against the same chain of oracles; the yardstick
is the chain run in np.float32 against the chain in float64 and PIPELINE_FACTOR32 is set from the measured ratio in the same way."""

from __future__ import annotations

import dataclasses
import functools

import numpy as np
import pytest

from tests import flux_ref as R
from tests import vae_ref as V
from tests.conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

g15 = load_golden("g15_flux.npz")
MEASURED = ("rel_err(gpu, ref64): 2.113e-7, ratio 0.623 (one timestep); 1.853e-7, 0.519 (a timestep per element); 1.945e-7, 0.608 "
            "(guidance); 1.694e-7, 0.474 (second step on the cached prompt); twice the worst is 1.246, hence FACTOR32 = 2 and a bar of "
            "7.15e-7.  Pipeline: rel_err 6.534e-7 against rel_err(ref32, ref64) 3.919e-7, ratio 1.667; twice it is 3.33, hence 4")
FACTOR32 = 2.0
PIPELINE_FACTOR32 = 4.0
CAP32 = 1e-4
BAR16 = 1e-2
NAMES = {"f32": "float32", "bf16": "bfloat16", "f16": "float16"}
CFG = R.fixture_config()
GUID_CFG = dataclasses.replace(CFG, guidance_embeds=True)
IDS = dict(img_ids=g15["img_ids"], txt_ids=g15["txt_ids"])


def _pk_config(cfg):
    from pygpukit_amd.diffusion import FluxConfig

    return FluxConfig(in_channels=cfg.in_channels, hidden_size=cfg.hidden_size, num_layers=cfg.num_layers,
                      num_single_layers=cfg.num_single_layers, num_attention_heads=cfg.num_attention_heads,
                      attention_head_dim=cfg.attention_head_dim, joint_attention_dim=cfg.joint_attention_dim,
                      pooled_projection_dim=cfg.pooled_projection_dim, guidance_embeds=cfg.guidance_embeds, axes_dims_rope=cfg.axes_dims_rope)


@functools.lru_cache(maxsize=None)
def _weights(guidance=False):
    return R.make_weights(GUID_CFG if guidance else CFG, int(g15["seed"]) + (10 if guidance else 0))


@functools.lru_cache(maxsize=None)
def _model(dtype, guidance=False):
    from pygpukit_amd.diffusion import FluxTransformer

    return FluxTransformer(_pk_config(GUID_CFG if guidance else CFG), _weights(guidance), dtype=NAMES[dtype])


@functools.lru_cache(maxsize=None)
def _ref64(dtype, key="out_t2", swap=False):
    guid = key == "out_guid"
    t = np.full(2, float(g15["timestep"]), np.float32) if key == "out" else g15["timesteps"]
    out = R.forward(GUID_CFG if guid else CFG, _weights(guid), g15["hidden"], g15["text"], g15["pooled"], t, g15["img_ids"][0],
                    g15["txt_ids"][0], guidance=g15["guidance"] if guid else None, round_dtype=dtype, swap_conditioning=swap)
    out.setflags(write=False)
    return out


def _yard(key="out_t2"):
    return rel_err(g15[key], _ref64("f32", key))


def _bar(dtype, key="out_t2"):
    return min(FACTOR32 * _yard(key), CAP32) if dtype == "f32" else BAR16


def _dev(a, dtype):
    from pygpukit_amd.core import from_numpy

    return from_numpy(R.to_words(R.round_to(a, dtype), dtype))


def _host(a, dtype):
    return R.from_words(a.to_numpy(), dtype).astype(np.float64)


def _run(model, dtype, hidden=None, timestep=None, text="fixture", pooled=None, guidance=None, ids=IDS):
    hidden = g15["hidden"] if hidden is None else hidden
    timestep = g15["timesteps"] if timestep is None else timestep
    if isinstance(text, str):
        text, pooled = g15["text"], g15["pooled"]
    out = model.forward(_dev(hidden, dtype), None if text is None else _dev(text, dtype), None if text is None else _dev(pooled, dtype),
                        timestep, guidance=guidance, **ids)
    assert out.shape == hidden.shape and out.dtype.name == NAMES[dtype]
    return _host(out, dtype)


@pytest.mark.parametrize("key", ["out", "out_t2", "out_guid"])
def test_float32_forward_against_the_reference_and_the_oracle(key):
    yard, bar = _yard(key), _bar("f32", key)
    assert 1e-7 < yard < 1e-6 and bar <= CAP32
    guid = key == "out_guid"
    got = _run(_model("f32", guid), "f32", timestep=float(g15["timestep"]) if key == "out" else None, guidance=g15["guidance"] if guid else None)
    e = rel_err(got, _ref64("f32", key))
    print(f"FLUX f32 {key}: rel_err(gpu, ref64) {e:.3e}, rel_err(fixture, ref64) {yard:.3e}, ratio {e / yard:.3f}, "
          f"rel_err(gpu, fixture) {rel_err(got, g15[key]):.3e} (MEASURED: {MEASURED})")
    assert np.isfinite(got).all() and e <= bar


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_16_bit_forward(dtype):
    from pygpukit_amd.diffusion import flux_plan

    model = _model(dtype)
    assert model.plan == flux_plan(model.config, NAMES[dtype])
    assert model.plan["attention"] == "flash" and model.plan["qk_norm_rope"] == "flux_qk_norm_rope_vec"
    assert model.mod_w.shape == ((12 * 2 + 3 * 2 + 2) * 128, 128) and model.double[0].qkv_w.shape == (384, 128)
    assert model.single[0].out_w.shape == (128, 640) and model.mod_w.dtype.name == NAMES[dtype]
    got = _run(model, dtype)
    e, e_fix = rel_err(got, _ref64(dtype)), rel_err(got, g15["out_t2"])
    print(f"FLUX {dtype}: rel_err vs the rounded-input oracle {e:.3e}, vs the reference's float32 fixture {e_fix:.3e}")
    assert np.isfinite(got).all() and e <= BAR16


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_swapped_conditioning_misses_the_bar(dtype):
    """Negative control: the oracle of a model that modulates each batch element with the other's conditioning must be rejected
    by the bar the right one passes - the bars see which row of the modulation projection a block reads."""
    got = _run(_model(dtype), dtype)
    wrong = rel_err(got, _ref64(dtype, swap=True))
    print(f"FLUX {dtype}: rel_err against the swapped-conditioning oracle {wrong:.3e}, bar {_bar(dtype):.3e}")
    assert rel_err(got, _ref64(dtype)) <= _bar(dtype) < wrong and wrong > 0.1


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_cached_encoder_states_and_rope_tables(dtype):
    """set_encoder_states + forward(hidden, timestep=...) is the full forward bit for bit; a second step at other timesteps
    reuses the prompt's projections and the cached tables and is right."""
    model = _model(dtype)
    full = _run(model, dtype)
    n, tables = model.encoder_projections, len(model._rope)
    model.set_encoder_states(_dev(g15["text"], dtype), _dev(g15["pooled"], dtype))
    assert model.encoder_projections == n + 1
    np.testing.assert_array_equal(_run(model, dtype, text=None), full)
    other = np.array([100.0, 900.0], np.float32)
    step2 = _run(model, dtype, timestep=other, text=None)
    assert model.encoder_projections == n + 1 and len(model._rope) == tables
    ref = R.forward(CFG, _weights(), g15["hidden"], g15["text"], g15["pooled"], other, g15["img_ids"][0], g15["txt_ids"][0], round_dtype=dtype)
    e = rel_err(step2, ref)
    print(f"FLUX {dtype} second step on the cached prompt: rel_err {e:.3e}" + (f", ratio {e / _yard():.3f}" if dtype == "f32" else ""))
    assert e <= _bar(dtype) and rel_err(step2, full) > 0.05
    np.testing.assert_array_equal(_run(model, dtype, timestep=other), step2)                # a fresh forward
    with pytest.raises(ValueError, match="batch"):
        _run(model, dtype, hidden=g15["hidden"][:1], text=None)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_batch_element_one_alone_equals_row_one_of_the_batch(dtype):
    model = _model(dtype)
    both = _run(model, dtype)
    alone = _run(model, dtype, hidden=g15["hidden"][1:], timestep=g15["timesteps"][1:], text=g15["text"][1:], pooled=g15["pooled"][1:])
    # the conditioning GEMMs see one row instead of two and may pick another kernel: the dtype's bar, not bit equality
    e = rel_err(alone[0], both[1])
    print(f"FLUX {dtype}: element 1 alone against row 1 of the batch: rel_err {e:.3e}, against the oracle "
          f"{rel_err(alone[0], _ref64(dtype)[1]):.3e}" + (f", ratio {rel_err(alone[0], _ref64(dtype)[1]) / _yard():.3f}" if dtype == "f32" else ""))
    assert e <= _bar(dtype) and rel_err(alone[0], _ref64(dtype)[1]) <= _bar(dtype) and rel_err(alone[0], both[0]) > 0.1


def test_ids_of_element_zero_serve_the_batch_and_default_ids():
    """[B, n, 3] ids: element 0's are used for every element (the reference's behaviour), so garbage in element 1's changes
    nothing; a square grid needs no ids."""
    model = _model("f32")
    img = g15["img_ids"].copy()
    img[1] += 7
    np.testing.assert_array_equal(_run(model, "f32", ids=dict(img_ids=img, txt_ids=g15["txt_ids"])), _run(model, "f32"))
    np.testing.assert_array_equal(_run(model, "f32", ids=dict(img_ids=g15["img_ids"][0], txt_ids=g15["txt_ids"][0])), _run(model, "f32"))
    with pytest.raises(ValueError, match="square"):
        _run(model, "f32", ids={})
    hidden = np.random.default_rng(3).standard_normal((2, 4, 8)).astype(np.float32)
    got = _run(model, "f32", hidden=hidden, ids={})
    ref = R.forward(CFG, _weights(), hidden, g15["text"], g15["pooled"], g15["timesteps"], R.image_ids(2, 2), R.text_ids(5))
    print(f"FLUX f32 default ids, a 2 x 2 grid: rel_err {rel_err(got, ref):.3e}, ratio {rel_err(got, ref) / _yard():.3f}")
    assert rel_err(got, ref) <= _bar("f32")


def test_from_safetensors_round_trip(tmp_path):
    from pygpukit_amd.diffusion import FluxTransformer
    from pygpukit_amd.llm.safetensors import save_safetensors

    save_safetensors(str(tmp_path / "diffusion_pytorch_model.safetensors"), {k: (v, "F32") for k, v in _weights(True).items()})
    model = FluxTransformer.from_safetensors(tmp_path, dtype="float32")
    assert model.config == _pk_config(GUID_CFG)
    np.testing.assert_array_equal(_run(model, "f32", guidance=g15["guidance"]), _run(_model("f32", True), "f32", guidance=g15["guidance"]))
    with pytest.raises(FileNotFoundError):
        FluxTransformer.from_safetensors(tmp_path / "not_there.safetensors")
    with pytest.raises(KeyError, match="proj_out.weight"):
        FluxTransformer(_pk_config(CFG), {k: v for k, v in _weights().items() if k != "proj_out.weight"})


def test_forward_needs_encoder_states_and_a_timestep():
    from pygpukit_amd.diffusion import FluxTransformer

    model = FluxTransformer(_pk_config(CFG), _weights(), dtype="float32")
    with pytest.raises(RuntimeError, match="encoder states"):
        model.forward(_dev(g15["hidden"], "f32"), timestep=g15["timesteps"], **IDS)
    with pytest.raises(ValueError, match="timestep"):
        model.forward(_dev(g15["hidden"], "f32"), _dev(g15["text"], "f32"), _dev(g15["pooled"], "f32"), **IDS)
    with pytest.raises(ValueError, match="go together"):
        model.forward(_dev(g15["hidden"], "f32"), _dev(g15["text"], "f32"), timestep=g15["timesteps"], **IDS)


def test_flux_plan_counts_the_launches_of_the_fixture():
    """No launch hook exists in the library (the VAE's plan is checked by formula too): the formula on the fixture's shape."""
    from pygpukit_amd.diffusion import flux_plan

    plan = flux_plan(_pk_config(CFG), "bfloat16", batch=2)
    assert (plan["launches_double"], plan["launches_single"]) == (16, 7)
    assert plan["launches_step"] == (3 + 1 + 1 + 1 + 1) + 2 * (1 + 1 + 2 + 2 * 16 + 2 * 7 + 1)


# ---- the pipeline -------------------------------------------------------------------------------------------------------------------
HEIGHT, WIDTH, STEPS = 32, 48, 2


def _vae_spec():
    from pygpukit_amd.diffusion import VAESpec

    return VAESpec(name="flux_fixture_vae", latent_channels=2, scaling_factor=0.5, block_out_channels=(8, 16, 16, 16), layers_per_block=1,
                   norm_num_groups=4, norm_eps=1e-6, shift_factor=0.25)


@functools.lru_cache(maxsize=None)
def _pipeline_oracle(dtype):
    from pygpukit_amd.diffusion.models.flux import FlowMatchEulerScheduler

    sched = FlowMatchEulerScheduler()
    sched.set_timesteps(STEPS)
    latents = np.random.default_rng(9).standard_normal((2, 6, 8)).astype(np.float32)
    x = R.sample_loop(CFG, _weights(), latents, g15["text"], g15["pooled"], sched.sigmas, R.image_ids(2, 3), R.text_ids(5), dtype=dtype)
    image = V.forward(_vae_spec(), V.make_weights(_vae_spec(), V.FIXTURE_SEED), R.unpack_latents(x, 2, 3), dtype)
    return latents, x, image


def test_two_step_pipeline_against_the_oracle_loop():
    from pygpukit_amd.diffusion import VAE, FluxPipeline

    latents, x64, image64 = _pipeline_oracle(np.float64)
    _, _, image32 = _pipeline_oracle(np.float32)
    yard = rel_err(image32, image64)
    bar = min(PIPELINE_FACTOR32 * yard, CAP32)
    vae = VAE(_vae_spec(), V.make_weights(_vae_spec(), V.FIXTURE_SEED), dtype="float32")
    pipe = FluxPipeline(_model("f32"), vae)
    image = pipe(_dev(g15["text"], "f32"), _dev(g15["pooled"], "f32"), HEIGHT, WIDTH, num_inference_steps=STEPS, latents=latents)
    assert image.shape == (2, 3, HEIGHT, WIDTH) and pipe.scheduler.step_index == STEPS
    got = image.to_numpy().astype(np.float64)
    e = rel_err(got, image64)
    print(f"FluxPipeline f32, {STEPS} steps: rel_err(gpu, ref64) {e:.3e}, rel_err(ref32, ref64) {yard:.3e}, ratio {e / yard:.3f}")
    assert np.isfinite(got).all() and np.abs(got).max() <= 1.0 and yard > 0 and e <= bar
    # the latents were stepped: the image of the noise itself is another image
    noise_image = V.forward(_vae_spec(), V.make_weights(_vae_spec(), V.FIXTURE_SEED), R.unpack_latents(latents.astype(np.float64), 2, 3))
    assert rel_err(noise_image, image64) > 0.05
    u8 = pipe.to_uint8(image)
    assert u8.shape == (2, HEIGHT, WIDTH, 3) and u8.dtype == np.uint8
    np.testing.assert_array_equal(u8, np.clip((image.to_numpy() + 1.0) / 2.0 * 255, 0, 255).astype(np.uint8).transpose(0, 2, 3, 1))
    # seed= draws the noise on the host with default_rng: the same seed gives the same image
    a = pipe(_dev(g15["text"], "f32"), _dev(g15["pooled"], "f32"), HEIGHT, WIDTH, num_inference_steps=1, seed=4).to_numpy()
    b = pipe(_dev(g15["text"], "f32"), _dev(g15["pooled"], "f32"), HEIGHT, WIDTH, num_inference_steps=1, seed=4).to_numpy()
    np.testing.assert_array_equal(a, b)
    with pytest.raises(ValueError, match="divisible by 16"):
        pipe(_dev(g15["text"], "f32"), _dev(g15["pooled"], "f32"), 40, WIDTH)
