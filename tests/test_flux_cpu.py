"""Host-side checks of the FLUX path: the oracle of tests/flux_ref.py against the reference's recorded float32 CPU outputs
(tests/golden/g15_flux.npz), the host tables, ids and scheduler numbers bit for bit, the pack / unpack restatement, the weight
packing, the launch arithmetic of flux_plan and the dispatch plan of flux_qk_norm_rope.  Nothing here needs a GPU.

Measured with the committed seeds: rel_err(fixture, ref64) = 3.39e-7 (one timestep), 3.57e-7 (a timestep per element), 3.20e-7
(guidance); rel_err(ref32, ref64) = 1.93e-7; the recorded joint / single attention and norm + rope cases are 2.9e-7 / 3.1e-7 /
2.8e-7 / 6.6e-8 from the float64 oracle.  The bars are a few float32 roundings deep: 2e-6 on a four-block forward, 1e-6 on one
attention (three GEMMs and a softmax deep), 5e-7 on a single op.

16-bit emulation (flux_ref.forward with round_activations: every activation rounded where the device stores it): 4.28e-3 in
bfloat16 and 4.5e-4 in float16 from the float64 oracle on the rounded weights and inputs, which is the oracle the GPU test holds
the device to with a bar of 1e-2; EMULATION_BAR = 5e-3 is half of that bar.  (Against the oracle on the UNROUNDED weights the
bfloat16 emulation lies 5.8e-3: rounding the weights and inputs alone moves this fixture by 3.1e-3.)"""

from __future__ import annotations

import dataclasses
import functools

import numpy as np
import pytest

from tests import flux_ref as R
from tests.conftest import load_golden, rel_err

g15 = load_golden("g15_flux.npz")
FORWARD_BAR = 2e-6
ATTN_BAR = 1e-6
OP_BAR = 5e-7
EMULATION_BAR = 5e-3
CFG = R.fixture_config()
GUID_CFG = dataclasses.replace(CFG, guidance_embeds=True)


@functools.lru_cache(maxsize=None)
def _weights(guidance=False):
    return R.make_weights(GUID_CFG if guidance else CFG, int(g15["seed"]) + (10 if guidance else 0))


@functools.lru_cache(maxsize=None)
def _forward(key: str, dtype, round_dtype="f32", round_activations=False):
    guid = key == "out_guid"
    t = np.full(2, float(g15["timestep"]), np.float32) if key == "out" else g15["timesteps"]
    out = R.forward(GUID_CFG if guid else CFG, _weights(guid), g15["hidden"], g15["text"], g15["pooled"], t, g15["img_ids"][0],
                    g15["txt_ids"][0], guidance=g15["guidance"] if guid else None, dtype=dtype, round_dtype=round_dtype,
                    round_activations=round_activations)
    out.setflags(write=False)
    return out


def _pk_config(cfg=CFG):
    from pygpukit_amd.diffusion import FluxConfig

    return FluxConfig(in_channels=cfg.in_channels, hidden_size=cfg.hidden_size, num_layers=cfg.num_layers,
                      num_single_layers=cfg.num_single_layers, num_attention_heads=cfg.num_attention_heads,
                      attention_head_dim=cfg.attention_head_dim, joint_attention_dim=cfg.joint_attention_dim,
                      pooled_projection_dim=cfg.pooled_projection_dim, guidance_embeds=cfg.guidance_embeds, axes_dims_rope=cfg.axes_dims_rope)


def test_fixture_inputs_are_the_committed_seeds():
    for got, name in zip(R.make_inputs(int(g15["seed"])), ("hidden", "text", "pooled")):
        np.testing.assert_array_equal(got, g15[name])
    assert int(g15["seed"]) == R.FIXTURE_SEED and g15["hidden"].shape == (2, 6, 8) and g15["text"].shape == (2, 5, 24)
    assert tuple(g15["timesteps"]) == R.FIXTURE_TIMESTEPS and float(g15["timestep"]) == R.FIXTURE_TIMESTEP
    assert tuple(g15["guidance"]) == R.FIXTURE_GUIDANCE


@pytest.mark.parametrize("key", ["out", "out_t2", "out_guid"])
def test_oracle_matches_the_reference_forward(key):
    e64, e32 = rel_err(g15[key], _forward(key, np.float64)), rel_err(g15[key], _forward(key, np.float32))
    print(f"{key}: rel_err(fixture, ref64) {e64:.3e}, rel_err(fixture, ref32) {e32:.3e}, "
          f"rel_err(ref32, ref64) {rel_err(_forward(key, np.float32), _forward(key, np.float64)):.3e}")
    assert g15[key].shape == (2, 6, 8) and np.isfinite(g15[key]).all()
    assert 1e-8 < e64 < FORWARD_BAR and e32 < FORWARD_BAR


def test_both_batch_elements_the_conditioning_and_the_guidance_matter():
    ref = _forward("out_t2", np.float64)
    swapped = R.forward(CFG, _weights(), g15["hidden"], g15["text"], g15["pooled"], g15["timesteps"], g15["img_ids"][0], g15["txt_ids"][0],
                        swap_conditioning=True)
    assert rel_err(swapped, ref) > 0.1
    assert rel_err(_forward("out", np.float64)[1], ref[1]) > 0.1           # element 1: timestep 750 against 250
    np.testing.assert_allclose(_forward("out", np.float64)[0], ref[0], rtol=0, atol=1e-12)
    no_guidance = R.forward(GUID_CFG, _weights(True), g15["hidden"], g15["text"], g15["pooled"], g15["timesteps"], g15["img_ids"][0],
                            g15["txt_ids"][0])
    assert rel_err(no_guidance, _forward("out_guid", np.float64)) > 0.1


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_16_bit_emulation_stays_within_half_the_gpu_bar(dtype):
    """The condition that makes the GPU test's 1e-2 meaningful: a device that rounds where this one does, and is otherwise exact,
    uses at most half of it."""
    oracle = _forward("out_t2", np.float64, dtype)
    emulated = _forward("out_t2", np.float64, dtype, True)
    e = rel_err(emulated, oracle)
    print(f"{dtype}: emulation against the rounded-input oracle {e:.3e}, against the unrounded oracle "
          f"{rel_err(emulated, _forward('out_t2', np.float64)):.3e}; rounding the weights and inputs alone "
          f"{rel_err(oracle, _forward('out_t2', np.float64)):.3e}")
    assert 0 < e <= EMULATION_BAR


def test_host_tables_and_ids_are_bit_identical_to_the_reference():
    from pygpukit_amd.diffusion.models.flux import embeddings as E

    img, txt = E.prepare_image_ids(2, *R.FIXTURE_GRID), E.prepare_text_ids(2, R.FIXTURE_TEXT_TOKENS)
    for got, name in ((img, "img_ids"), (txt, "txt_ids")):
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, g15[name])
    np.testing.assert_array_equal(R.image_ids(*R.FIXTURE_GRID), g15["img_ids"][0])
    np.testing.assert_array_equal(R.text_ids(R.FIXTURE_TEXT_TOKENS), g15["txt_ids"][0])
    cos, sin = E.get_rope_frequencies(img[0], txt[0], axes_dim=CFG.axes_dims_rope)
    assert cos.dtype == sin.dtype == np.float32 and cos.shape == (11, 64)
    np.testing.assert_array_equal(cos, g15["rope_cos"])
    np.testing.assert_array_equal(sin, g15["rope_sin"])
    # text rows first; every table value sits on both elements of its pair; axis 0 of the ids fills the first 16 columns
    np.testing.assert_array_equal(cos[:, 0::2], cos[:, 1::2])
    assert (cos[:5, 16:] == 1).all() and (sin[:5, 16:] == 0).all() and (cos[5:, :16] == 1).all() and not (sin[6:, 16:] == 0).all()
    c64, s64 = R.rope_tables(np.concatenate([txt[0], img[0]]), CFG.axes_dims_rope)
    assert np.abs(c64 - g15["rope_cos"]).max() <= 2 ** -23 and np.abs(s64 - g15["rope_sin"]).max() <= 2 ** -23
    t = E.timestep_embedding(g15["timesteps"], 256)
    assert t.dtype == np.float32
    np.testing.assert_array_equal(t, g15["t_emb"])
    np.testing.assert_array_equal(R.timestep_embedding(g15["timesteps"]), g15["t_emb"])
    assert E.timestep_embedding(np.array([0.5], np.float32), 7).shape == (1, 7)
    assert E.__all__ == ["get_1d_rotary_pos_embed", "get_rope_frequencies", "apply_rope", "timestep_embedding", "prepare_image_ids",
                         "prepare_text_ids"]


def test_norm_rope_and_attention_oracles_match_the_reference():
    from pygpukit_amd.diffusion.models.flux.embeddings import apply_rope

    nr64 = R.qk_norm_rope(g15["nr_x"], g15["nr_w"], None, 11, g15["nr_cos"], g15["nr_sin"])
    nr32 = R.qk_norm_rope(g15["nr_x"], g15["nr_w"], None, 11, g15["nr_cos"], g15["nr_sin"], dtype=np.float32)
    assert rel_err(g15["nr_out"], nr64) < OP_BAR and rel_err(nr32, nr64) < OP_BAR
    # the table is a general one: the two elements of a pair carry different values
    assert not np.array_equal(g15["nr_cos"][:, 0::2], g15["nr_cos"][:, 1::2])
    normed = R.rms_norm(g15["nr_x"].astype(np.float64), g15["nr_w"].astype(np.float64))
    np.testing.assert_allclose(apply_rope(normed, g15["nr_cos"].astype(np.float64), g15["nr_sin"].astype(np.float64)), nr64, rtol=0, atol=1e-12)
    for wrong in (dict(pairing="half"), dict(global_row=True)):
        tabs = (np.tile(g15["nr_cos"], (2, 1)), np.tile(g15["nr_sin"], (2, 1))) if "global_row" in wrong else (g15["nr_cos"], g15["nr_sin"])
        bad = R.qk_norm_rope(g15["nr_x"], g15["nr_w"], None, 11, *tabs, **wrong)
        # global_row on a table tiled per batch element is the right answer again: the control needs a table that differs
        assert (rel_err(bad, nr64) > 0.1) == ("pairing" in wrong)
    case = R.make_attention_case(int(g15["seed"]) + 3)
    img, txt = R.joint_attention(case, g15["ja_cos"], g15["ja_sin"])
    single = R.joint_attention(case, g15["ja_cos"], g15["ja_sin"], single=True)
    errs = rel_err(g15["ja_out_img"], img), rel_err(g15["ja_out_txt"], txt), rel_err(g15["sa_out"], single)
    print("joint image / joint text / single attention against the oracle:", errs)
    assert max(errs) < ATTN_BAR and g15["sa_out"].shape == (2, 7, 128)


def test_scheduler_numbers_are_bit_identical_to_the_reference():
    from pygpukit_amd.diffusion.models.flux import FlowMatchEulerScheduler, FlowMatchEulerSchedulerConfig

    def sched(steps, mu_len=None, **kw):
        s = FlowMatchEulerScheduler(FlowMatchEulerSchedulerConfig(**kw))
        with np.errstate(divide="ignore"):
            s.set_timesteps(steps, mu=None if mu_len is None else s.compute_mu(mu_len))
        return s

    cases = {"4_1": sched(4), "5_3": sched(5, shift=3.0), "dyn256": sched(4, 256, use_dynamic_shifting=True),
             "dyn4096": sched(4, 4096, use_dynamic_shifting=True)}
    for name, s in cases.items():
        assert s.sigmas.dtype == s.timesteps.dtype == np.float32 and s.step_index == 0
        np.testing.assert_array_equal(s.sigmas, g15["sched_sigmas_" + name])
        np.testing.assert_array_equal(s.timesteps, g15["sched_timesteps_" + name])
    np.testing.assert_array_equal(R.scheduler_sigmas(5, 3.0), g15["sched_sigmas_5_3"])
    np.testing.assert_array_equal(R.scheduler_sigmas(4, mu=R.scheduler_mu(4096)), g15["sched_sigmas_dyn4096"])
    np.testing.assert_array_equal([sched(1).compute_mu(n) for n in (256, 1024, 4096)], g15["sched_mu"])
    assert g15["sched_mu"][0] == 0.5 and abs(g15["sched_mu"][2] - 1.15) < 1e-12
    # without mu dynamic shifting changes nothing, as in the reference
    np.testing.assert_array_equal(sched(4, use_dynamic_shifting=True).sigmas, g15["sched_sigmas_4_1"])
    s, x = sched(4), g15["sched_sample"]
    for i, t in enumerate(s.timesteps):
        x = s.step(g15["sched_velocity"][i], t, x)
        assert x.dtype == np.float32 and s.step_index == i + 1
        np.testing.assert_array_equal(x, g15["sched_trajectory"][i])
    with pytest.raises(ValueError, match="set_timesteps"):
        FlowMatchEulerScheduler().step(x, 0.0, x)
    np.testing.assert_array_equal(s.add_noise(x, 2 * x, 0.25), ((1 - 0.25) * x + 0.25 * (2 * x)).astype(np.float32))
    assert s.scale_model_input(x) is x


def test_pack_and_unpack_restatements():
    np.testing.assert_array_equal(R.unpack_latents(g15["unpack_in"], 2, 3), g15["unpack_out"])
    np.testing.assert_array_equal(R.pack_latents(g15["unpack_out"]), g15["unpack_in"])
    assert g15["unpack_out"].shape == (2, 16, 4, 6)
    # column c * 4 + ph * 2 + pw of token (y, x) is pixel (2y + ph, 2x + pw) of channel c
    assert g15["unpack_out"][1, 5, 2 * 1 + 1, 2 * 2 + 0] == g15["unpack_in"][1, 1 * 3 + 2, 5 * 4 + 1 * 2 + 0]


def test_weight_packing_helpers():
    from pygpukit_amd.diffusion.models.flux.model import modulation_layout, modulation_names, pack_qkv

    w, cfg, D = _weights(), _pk_config(), CFG.hidden_size
    qkv = pack_qkv(w, "transformer_blocks.1.attn")
    assert qkv.shape == (3 * D, D)
    for i, n in enumerate(("to_q", "to_k", "to_v")):
        np.testing.assert_array_equal(qkv[i * D:(i + 1) * D], w[f"transformer_blocks.1.attn.{n}.weight"])
    added = pack_qkv(w, "transformer_blocks.0.attn", ("add_q_proj", "add_k_proj", "add_v_proj"), "bias")
    np.testing.assert_array_equal(added[D:2 * D], w["transformer_blocks.0.attn.add_k_proj.bias"])
    lay, names = modulation_layout(cfg), modulation_names(cfg)
    assert lay["rows"] == (12 * 2 + 3 * 2 + 2) * D and lay["double"] == [(0, 6 * D), (12 * D, 18 * D)]
    assert lay["single"] == [24 * D, 27 * D] and lay["out"] == 30 * D
    assert names == ["transformer_blocks.0.norm1.linear", "transformer_blocks.0.norm1_context.linear", "transformer_blocks.1.norm1.linear",
                     "transformer_blocks.1.norm1_context.linear", "single_transformer_blocks.0.norm.linear",
                     "single_transformer_blocks.1.norm.linear", "norm_out.linear"]
    # the offsets are where each layer's rows start in the stack of `names`
    starts = np.cumsum([0] + [w[n + ".weight"].shape[0] for n in names])
    assert list(starts[:-1]) == [lay["double"][0][0], lay["double"][0][1], lay["double"][1][0], lay["double"][1][1], *lay["single"], lay["out"]]
    assert starts[-1] == lay["rows"]
    full = modulation_layout(type(cfg)())
    assert full["rows"] == (12 * 19 + 3 * 38 + 2) * 3072 and len(full["double"]) == 19 and len(full["single"]) == 38


def test_flux_plan_launch_arithmetic():
    from pygpukit_amd.diffusion import FluxConfig, flux_plan

    plan = flux_plan(FluxConfig(), "bfloat16")
    assert plan["launches_double"] == 16 and plan["launches_single"] == 7
    assert plan["attention"] == "flash" and plan["qk_norm_rope"] == "flux_qk_norm_rope_vec"
    # conditioning 3 + 1 + silu + cast + GEMM; x_embedder, text copy, two first norms; the blocks; proj_out
    assert plan["launches_step"] == 7 + 4 + 19 * 16 + 38 * 7 + 1 == 582
    assert flux_plan(FluxConfig(), "float32")["launches_step"] == 581 and flux_plan(FluxConfig(), "float32")["attention"] == "fallback"
    assert flux_plan(FluxConfig(guidance_embeds=True), "bfloat16")["launches_step"] == 586
    fix = flux_plan(_pk_config(), "float16", batch=2)
    assert fix["launches_step"] == 7 + 2 * (4 + 2 * 16 + 2 * 7 + 1) and fix["qk_norm_rope"] == "flux_qk_norm_rope_vec"
    odd = FluxConfig(hidden_size=144, num_attention_heads=2, attention_head_dim=72, axes_dims_rope=(16, 28, 28))
    assert flux_plan(odd, "bfloat16") ["qk_norm_rope"] == "flux_qk_norm_rope_scalar" and flux_plan(odd, "bfloat16")["attention"] == "fallback"


def test_qk_norm_rope_plan_on_every_branch_and_its_errors():
    from pygpukit_amd import _hip
    from pygpukit_amd.diffusion.ops import flux_qk_norm_rope_plan

    for dtype in ("float32", "bfloat16", "float16"):
        for hd in (64, 128):
            assert flux_qk_norm_rope_plan(hd, dtype) == "flux_qk_norm_rope_vec"
            assert flux_qk_norm_rope_plan(hd, dtype, aligned=False) == "flux_qk_norm_rope_scalar"
        for hd in (2, 6, 32, 72, 96, 256):
            assert flux_qk_norm_rope_plan(hd, dtype) == "flux_qk_norm_rope_scalar"
    for hd in (7, 127, 0, -2, 258):
        with pytest.raises(ValueError, match="head_dim"):
            flux_qk_norm_rope_plan(hd, "bfloat16")
    with pytest.raises(ValueError, match="dtype"):
        flux_qk_norm_rope_plan(64, "int32")
    lib = _hip.load()
    for name in ("pgk_flux_qk_norm_rope", "pgk_flux_qk_norm_rope_plan", "pgk_flux_gelu_pack", "pgk_flux_unpack_latents", "pgk_flow_euler_step"):
        assert name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name)


def test_public_names_and_the_pipeline_without_text_encoders():
    from pygpukit_amd import diffusion
    from pygpukit_amd.diffusion.models import flux

    assert flux.__all__[:5] == ["FluxTransformer", "FluxConfig", "FlowMatchEulerScheduler", "FlowMatchEulerSchedulerConfig", "FluxPipeline"]
    for name in flux.__all__:
        assert getattr(flux, name) is getattr(diffusion, name) and name in diffusion.__all__
    cfg = flux.FluxConfig()
    assert (cfg.in_channels, cfg.out_channels, cfg.hidden_size, cfg.num_layers, cfg.num_single_layers, cfg.num_attention_heads,
            cfg.attention_head_dim, cfg.joint_attention_dim, cfg.pooled_projection_dim, cfg.guidance_embeds, cfg.axes_dims_rope,
            cfg.head_dim) == (64, None, 3072, 19, 38, 24, 128, 4096, 768, False, (16, 56, 56), 128)
    with pytest.raises(NotImplementedError, match="prompt_embeds"):
        flux.FluxPipeline.from_pretrained("somewhere")
    pipe = flux.FluxPipeline.__new__(flux.FluxPipeline)
    with pytest.raises(NotImplementedError, match="prompt_embeds"):
        pipe.encode_prompt("a cat")
    with pytest.raises(NotImplementedError, match="prompt_embeds"):
        pipe("a cat")
    detected = flux.FluxTransformer._detect_config(_weights(True))
    assert detected == _pk_config(GUID_CFG)
