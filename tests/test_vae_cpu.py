"""conv2d, group_norm and the VAE decoder without a GPU: the NumPy oracle (tests/vae_ref.py) against the reference's CPU ops and a
torch float64 restatement of the decoder (tests/golden/g14_vae.npz), how far wrong decoders land from the right one, the
exports, the argument errors raised before the device is touched, the host-side plans and the safetensors reader.

Two bounds for the oracle.  The torch records are float64, and the oracle is held to them at 1e-12.  The reference's own CPU
conv2d / group_norm compute in float32, so their records cannot be met at 1e-12 by any float64 oracle: they are held at float32's
own distance - 4e-7 of sum |x w| + |b| per element for conv2d (n 2^-24 with n <= 361 would allow 2e-5; measured 1e-7), 5e-6
absolute for group_norm on O(1) outputs.  The float64 anchor covers conv cases 2-7 and group-norm cases 0-2 (the fixture stays
small); conv cases 0 and 1 are anchored by the reference's float32 record of case 1 and by sharing the code path of the others."""

from __future__ import annotations

import numpy as np
import pytest

from tests import vae_ref as R
from tests.conftest import load_golden

g14 = load_golden("g14_vae.npz")
NEW_ENTRIES = ("pgk_conv2d", "pgk_conv2d_plan", "pgk_conv2d_packed_elems", "pgk_conv2d_pack_weight", "pgk_group_norm", "pgk_group_norm_plan")
WIDEST_GPU_BAR = 4 * 1.2e-2          # FACTOR16's ceiling x the largest 16-bit floor (bfloat16, measured below)


def test_fixture_was_recorded_from_these_inputs():
    assert int(g14["seed"]) == R.FIXTURE_SEED and g14["dec"].shape == (2, 3, 20, 28)


@pytest.mark.parametrize("i", [int(i) for i in g14["ref_conv"]])
def test_conv2d_oracle_matches_the_reference(i):
    """The reference's CPU conv2d is float32: its distance to the float64 sum is float32's, a few 1e-7 of the magnitude."""
    x, w, b = R.conv_inputs(i)
    s, p, d = R.CONV_CASES[i][6:9]
    want = g14[f"conv_{i}"]
    got = R.conv2d(x, w, b, s, p, d)
    assert got.shape == want.shape
    assert np.max(np.abs(got - want) / R.conv2d(x, w, b, s, p, d, absolute=True)) <= 4e-7


@pytest.mark.parametrize("i", [int(i) for i in g14["torch_conv"]])
def test_conv2d_oracle_matches_torch_float64(i):
    x, w, b = R.conv_inputs(i)
    s, p, d = R.CONV_CASES[i][6:9]
    assert np.max(np.abs(R.conv2d(x, w, b, s, p, d) - g14[f"tconv_{i}"])) <= 1e-12


@pytest.mark.parametrize("i", [int(i) for i in g14["ref_gn"]])
def test_group_norm_oracle_matches_the_reference(i):
    x, gamma, beta = R.gn_inputs(i)
    groups = R.GN_CASES[i][4]
    assert np.max(np.abs(R.group_norm(x, gamma, beta, groups, 1e-5) - g14[f"gn_{i}"])) <= 5e-6
    assert np.max(np.abs(R.group_norm(x, gamma, beta, groups, 1e-5, silu=True) - g14[f"gns_{i}"])) <= 5e-6


@pytest.mark.parametrize("i", [int(i) for i in g14["torch_gn"]])
def test_group_norm_oracle_matches_torch_float64(i):
    x, gamma, beta = R.gn_inputs(i)
    assert np.max(np.abs(R.group_norm(x, gamma, beta, R.GN_CASES[i][4], 1e-5) - g14[f"tgn_{i}"])) <= 1e-12


def test_decoder_oracle_matches_torch_float64():
    spec, latent = R.fixture_spec(), R.make_latent(R.FIXTURE_SEED)
    w = R.make_weights(spec, R.FIXTURE_SEED)
    assert np.max(np.abs(R.forward(spec, w, latent) - g14["dec"])) <= 1e-12
    assert np.max(np.abs(R.forward(spec, R.make_weights(spec, R.FIXTURE_SEED, post_quant=False), latent) - g14["dec_nopq"])) <= 1e-12
    shifted = R.forward(R.fixture_spec(float(g14["shift"])), w, latent)
    assert np.max(np.abs(shifted - g14["dec_shift"])) <= 1e-12
    assert R.rel_err(g14["dec_shift"], g14["dec"]) > 1e-2 and R.rel_err(g14["dec_nopq"], g14["dec"]) > 1e-2
    assert (np.abs(g14["dec"]) == 1.0).any()                      # the clamp acts on the fixture


def test_sixteen_bit_floors_and_the_float32_yard():
    """The figures the GPU bars are built from, recomputed with NumPy (INTEGRATION.md quotes them)."""
    spec, latent = R.fixture_spec(), R.make_latent(R.FIXTURE_SEED)
    w = R.make_weights(spec, R.FIXTURE_SEED)
    floors = {}
    for dt in ("bfloat16", "float16"):
        floors[dt] = R.rel_err(R.forward(spec, w, latent, round_dtype=dt, round_activations=True), R.forward(spec, w, latent, round_dtype=dt))
    yard = R.rel_err(R.forward(spec, w, latent, dtype=np.float32), R.forward(spec, w, latent))
    print(f"floors {floors}, float32 yard {yard:.3e}")
    assert 3e-3 < floors["bfloat16"] < 1.2e-2 and 3e-4 < floors["float16"] < 2e-3 and 5e-8 < yard < 2e-6


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_a_wrong_decoder_lands_far_outside_the_widest_gpu_bar(mutation):
    spec, latent = R.fixture_spec(), R.make_latent(R.FIXTURE_SEED)
    w = R.make_weights(spec, R.FIXTURE_SEED)
    assert R.rel_err(R.forward(spec, w, latent, mutate=mutation), g14["dec"]) > 5 * WIDEST_GPU_BAR


def test_wrong_ops_land_far_outside_their_bars():
    """An ignored stride and a group boundary shifted by one channel, on the op cases themselves."""
    x, w, b = R.conv_inputs(4)                                     # stride 2
    right = R.conv2d(x, w, b, 2, 1)
    assert R.rel_err(R.conv2d(x, w, b, 1, 1)[:, :, ::2, ::2][:, :, :right.shape[2], :right.shape[3]], right) < 1e-12   # the subsampling identity
    assert R.rel_err(R.conv2d(x, w, b, 1, 1)[:, :, :right.shape[2], :right.shape[3]], right) > 0.5                     # stride ignored
    x, gamma, beta = R.gn_inputs(2)                                # 5 channels per group
    right = R.group_norm(x, gamma, beta, 2)
    wrong = np.roll(R.group_norm(np.roll(x, 1, axis=1), gamma, beta, 2), -1, axis=1)
    assert R.rel_err(wrong, right) > 0.05


def test_one_pass_variance_cannot_pass_the_stable_case():
    """The case tests/test_group_norm_gpu.py runs, same inputs (vae_ref.gn_stable_inputs)."""
    g = R.GN_STABLE_CASE[4]
    x, gamma, beta = R.gn_stable_inputs()
    ref = R.group_norm(x, gamma, beta, g)
    yard = np.abs(R.group_norm(x, gamma, beta, g, dtype=np.float32) - ref).max()
    one_pass = np.abs(R.group_norm_one_pass(x, gamma, beta, g) - ref).max()
    print(f"two-pass float32 yard {yard:.3e}, one-pass error {one_pass:.3e} ({one_pass / yard:.0f} x)")
    assert one_pass > 4 * 32 * yard                                # 32: the ceiling of FACTOR32 on this case


def test_exports():
    import pygpukit_amd as pk
    from pygpukit_amd import _hip, diffusion, ops
    from pygpukit_amd.diffusion import config
    from pygpukit_amd.ops import conv, nn
    from pygpukit_amd.ops.nn import norm

    assert pk.conv2d is ops.conv2d is conv.conv2d and "conv2d" in ops.__all__ and "conv2d" in conv.__all__
    for name in ("group_norm", "group_norm_silu"):
        assert getattr(pk, name) is getattr(ops, name) is getattr(nn, name) is getattr(norm, name)
        assert name in nn.__all__ and name in ops.__all__
    assert len(set(nn.__all__)) == len(nn.__all__) and len(set(ops.__all__)) == len(ops.__all__)
    for name in ("VAE", "VAESpec", "SDXL_VAE_SPEC", "SD3_VAE_SPEC", "FLUX_VAE_SPEC", "vae_plan"):
        assert name in diffusion.__all__ and hasattr(diffusion, name)
    # the ops live in pygpukit_amd.ops: diffusion.ops keeps the surface its own test pins
    for name in ("group_norm", "conv2d", "conv2d_transpose"):
        assert not hasattr(diffusion.ops, name)
    lib = _hip.load()
    for name in NEW_ENTRIES:
        assert name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name)
    s = config.SDXL_VAE_SPEC
    assert (s.latent_channels, s.scaling_factor, s.block_out_channels, s.layers_per_block, s.norm_num_groups, s.norm_eps, s.shift_factor) == \
        (4, 0.13025, (128, 256, 512, 512), 2, 32, 1e-6, 0.0)
    assert (config.SD3_VAE_SPEC.latent_channels, config.SD3_VAE_SPEC.scaling_factor) == (16, 1.5305)
    assert (config.FLUX_VAE_SPEC.latent_channels, config.FLUX_VAE_SPEC.scaling_factor) == (16, 0.3611)
    assert config.VAESpec(name="x").scaling_factor == 0.18215 and config.VAESpec(name="x").in_channels == 3


class _Fake:
    """Shape and dtype only: every check below must fire before a pointer is needed."""

    def __init__(self, shape, dtype="float32"):
        from pygpukit_amd.core.dtypes import as_dtype

        self.shape, self.ndim, self.dtype = tuple(shape), len(shape), as_dtype(dtype)


def test_conv2d_argument_errors_come_before_the_device():
    from pygpukit_amd.ops.conv import conv2d, conv2d_pack_weight

    x, w = _Fake((1, 8, 9, 9)), _Fake((4, 8, 3, 3))
    with pytest.raises(NotImplementedError, match="groups"):
        conv2d(x, w, groups=2)
    with pytest.raises(ValueError, match="4D"):
        conv2d(_Fake((8, 9, 9)), w)
    with pytest.raises(ValueError, match="in_channels"):
        conv2d(x, _Fake((4, 7, 3, 3)))
    with pytest.raises(ValueError, match="in_channels"):
        conv2d(x, w, channels_last=True)                       # [N, H, W, C]: 9 channels there
    with pytest.raises(ValueError, match="dtype"):
        conv2d(x, _Fake((4, 8, 3, 3), "bfloat16"))
    with pytest.raises(ValueError, match="bias"):
        conv2d(x, w, _Fake((5,)))
    with pytest.raises(ValueError, match="pair"):
        conv2d(x, w, stride=(1, 2, 3))
    with pytest.raises(ValueError, match="stride"):
        conv2d(x, w, stride=0)
    with pytest.raises(ValueError, match="empty"):
        conv2d(x, _Fake((4, 8, 11, 11)))
    with pytest.raises(ValueError, match="upsample"):
        conv2d(x, w, upsample=3)
    with pytest.raises(ValueError, match="add"):
        conv2d(x, w, padding=1, add=_Fake((1, 4, 9, 8)))
    with pytest.raises(ValueError, match="packed_weight"):
        conv2d(x, w, packed_weight=_Fake((9, 64, 32)))          # float32 reads no packed weight
    with pytest.raises(ValueError, match="float16/bfloat16"):
        conv2d_pack_weight(w)
    with pytest.raises(ValueError, match="4D"):
        conv2d_pack_weight(_Fake((4, 8, 3), "bfloat16"))


def test_group_norm_argument_errors_come_before_the_device():
    from pygpukit_amd.ops.nn.norm import group_norm, group_norm_plan, group_norm_silu

    x, g, b = _Fake((1, 8, 4, 4)), _Fake((8,)), _Fake((8,))
    with pytest.raises(ValueError, match="divisible"):
        group_norm(x, g, b, 3)
    with pytest.raises(ValueError, match="4D"):
        group_norm_silu(_Fake((8, 4, 4)), g, b, 2)
    with pytest.raises(ValueError, match="gamma"):
        group_norm(x, _Fake((4,)), b, 2)
    with pytest.raises(ValueError, match="gamma"):
        group_norm(x, g, b, 2, channels_last=True)             # 4 channels in that layout
    with pytest.raises(ValueError, match="dtype"):
        group_norm(x, _Fake((8,), "float16"), b, 2)
    with pytest.raises(ValueError, match="divisible"):
        group_norm_plan(1, 8, 16, 3)


def test_plans(monkeypatch):
    from pygpukit_amd.diffusion import SD3_VAE_SPEC, SDXL_VAE_SPEC, vae_plan
    from pygpukit_amd.ops.conv import conv2d_plan
    from pygpukit_amd.ops.nn.norm import group_norm_plan

    monkeypatch.delenv("PGK_CONV_MFMA", raising=False)
    monkeypatch.delenv("PGK_GN_SPLIT", raising=False)
    for i, c in enumerate(R.CONV_CASES):
        assert conv2d_plan(c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], "bfloat16") == R.CONV_PLANS_16[i]
        assert conv2d_plan(c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], "float32") == "fma"
    assert conv2d_plan(8, 8, 9, 9, (3, 1), 1, 1, 1, "float16") == "fma"          # not square
    assert conv2d_plan(8, 8, 9, 9, 3, (1, 2), 1, 1, "float16") == "fma"          # unequal strides
    assert conv2d_plan(8, 8, 9, 9, 3, 3, 1, 1, "float16") == "fma"               # stride 3
    assert conv2d_plan(512, 512, 64, 64, 3, 1, 1, 1, "bfloat16", upsample=2) == "mfma"
    monkeypatch.setenv("PGK_CONV_MFMA", "0")
    assert conv2d_plan(512, 512, 64, 64, 3, 1, 1, 1, "bfloat16") == "fma"
    monkeypatch.delenv("PGK_CONV_MFMA")
    assert group_norm_plan(1, 128, 1 << 20, 32, "bfloat16", True) == "split" and group_norm_plan(1, 32, 256, 4) == "block"
    monkeypatch.setenv("PGK_GN_SPLIT", "0")
    assert group_norm_plan(1, 128, 1 << 20, 32) == "block"
    monkeypatch.delenv("PGK_GN_SPLIT")

    p = vae_plan(SDXL_VAE_SPEC, "bfloat16", (128, 128))
    # 2 casts + div; post_quant_conv, conv_in; 2 mid resnets x 4; attention 5 + 4; up blocks (4+4+4) + (4+4+4) + (5+4+4) + (5+4+4);
    # 3 upsamplers; conv_norm_out, conv_out, clamp
    assert p["launches"] == 3 + 2 + 8 + 9 + 50 + 3 + 3 == 78 and p["attention"] == "matmul" and p["tokens"] == 16384
    assert p["scores_bytes"] == 16384 * 16384 * 2 and p["output_shape"] == (1, 3, 1024, 1024)
    assert p["conv"] == "mfma" and p["group_norm"] == "split"
    small = vae_plan(SDXL_VAE_SPEC, "float32", (8, 8), post_quant=False, batch=2)
    assert small["attention"] == "sdpa" and small["scores_bytes"] == 0 and small["conv"] == "fma"
    assert small["launches"] == 1 + 1 + 8 + 6 + 50 + 3 + 3
    assert vae_plan(SDXL_VAE_SPEC, "float32", (8, 8), "matmul")["attention"] == "matmul"
    # the measured thresholds: float32 takes the fallback kernel up to 256 tokens, the 16-bit dtypes never do on their own
    assert [vae_plan(SDXL_VAE_SPEC, "float32", hw)["attention"] for hw in ((16, 16), (16, 17), (32, 32))] == ["sdpa", "matmul", "matmul"]
    assert [vae_plan(SDXL_VAE_SPEC, dt, (8, 8))["attention"] for dt in ("bfloat16", "float16")] == ["matmul", "matmul"]
    assert vae_plan(SDXL_VAE_SPEC, "bfloat16", (8, 8), "sdpa")["attention"] == "sdpa"
    assert vae_plan(SD3_VAE_SPEC, "float16", (64, 64))["output_shape"] == (1, 3, 512, 512)
    with pytest.raises(ValueError, match="15360"):
        vae_plan(SDXL_VAE_SPEC, "bfloat16", (128, 128), "sdpa")
    with pytest.raises(ValueError, match="attention"):
        vae_plan(SDXL_VAE_SPEC, "bfloat16", (8, 8), "flash")


def test_vae_constructor_errors():
    from pygpukit_amd.diffusion import VAE

    spec = R.fixture_spec()
    with pytest.raises(ValueError, match="no weights"):
        VAE(spec)
    with pytest.raises(ValueError, match="attention"):
        VAE(spec, {"x": 1}, attention="flash")


def test_read_safetensors_selects_the_decoder_and_detects_the_spec(tmp_path):
    """The host side of VAE.from_safetensors: the directory search order, the encoder and the encoder-side quant_conv dropped,
    post_quant_conv kept, bfloat16 widened exactly, the spec from decoder.conv_in's input channels."""
    from pygpukit_amd.diffusion import SD3_VAE_SPEC, SDXL_VAE_SPEC, VAE
    from pygpukit_amd.llm.safetensors import save_safetensors

    spec = R.fixture_spec()
    w = R.make_weights(spec, R.FIXTURE_SEED)
    tensors = {k: (v, "F32") for k, v in w.items()}
    bf = (w["decoder.conv_out.bias"].view(np.uint32) >> 16).astype(np.uint16)
    tensors["decoder.conv_out.bias"] = (bf, "BF16")
    tensors["encoder.conv_in.weight"] = (np.ones((4, 3, 3, 3), np.float32), "F32")
    tensors["quant_conv.weight"] = (np.ones((8, 8, 1, 1), np.float32), "F32")
    d = tmp_path / "model"
    d.mkdir()
    save_safetensors(str(d / "zz_other.safetensors"), {"decoder.conv_in.weight": (np.zeros((8, 16, 3, 3), np.float32), "F32")})
    assert VAE.find_safetensors(d).name == "zz_other.safetensors"
    assert VAE.read_safetensors(d)[0] is SD3_VAE_SPEC                                    # 16 latent channels
    save_safetensors(str(d / "my_vae_fp16.safetensors"), tensors)
    assert VAE.find_safetensors(d).name == "my_vae_fp16.safetensors"                     # *vae* before any other file
    save_safetensors(str(d / "diffusion_pytorch_model.safetensors"), tensors)
    assert VAE.find_safetensors(d).name == "diffusion_pytorch_model.safetensors"
    save_safetensors(str(d / "vae.safetensors"), tensors)
    assert VAE.find_safetensors(d).name == "vae.safetensors" and VAE.find_safetensors(d / "my_vae_fp16.safetensors").name == "my_vae_fp16.safetensors"
    got_spec, got = VAE.read_safetensors(d)
    assert got_spec is SDXL_VAE_SPEC                                                     # 4 latent channels
    assert set(got) == set(w) and "post_quant_conv.weight" in got
    for k, v in w.items():
        want = (bf.astype(np.uint32) << 16).view(np.float32) if k == "decoder.conv_out.bias" else v
        assert got[k].dtype == np.float32 and np.array_equal(got[k], want), k
    assert VAE.read_safetensors(d, spec)[0] is spec
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(FileNotFoundError):
        VAE.find_safetensors(empty)
