"""Host-side checks of the diffusion-transformer path: the oracle of tests/dit_ref.py against the reference's recorded float32 CPU
outputs (tests/golden/g13_pixart.npz), the host tables bit for bit, the padded-head identity, the dispatch plan and the weight
packing.  Nothing here needs a GPU.

Measured with the committed seeds: rel_err(fixture, ref64) = 4.09e-7 for the scalar-timestep forward and 3.98e-7 for the
per-element one; rel_err(ref32, ref64) = 3.30e-7; the recorded adaln / adaln_zero / cross_attention cases are 6.1e-8 / 4.5e-8 /
6.1e-8 from the float64 oracle.  The bars below are a few float32 roundings deep: 2e-6 on a two-block forward (some hundred
float32 operations deep per output, each rounding <= 6e-8 relative), 5e-7 on a single op."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from tests import dit_ref as R
from tests.conftest import load_golden, rel_err

g13 = load_golden("g13_pixart.npz")
FORWARD_BAR = 2e-6
OP_BAR = 5e-7


@functools.lru_cache(maxsize=None)
def _weights():
    return R.make_weights(R.fixture_spec(), int(g13["seed"]))


@functools.lru_cache(maxsize=None)
def _forward(key: str, dtype):
    t = float(g13["timestep"]) if key == "out" else g13["timesteps"]
    out = R.forward(R.fixture_spec(), _weights(), g13["latent"], t, g13["text"], dtype)
    out.setflags(write=False)
    return out


def test_fixture_inputs_are_the_committed_seeds():
    latent, text = R.make_inputs(int(g13["seed"]))
    np.testing.assert_array_equal(latent, g13["latent"])
    np.testing.assert_array_equal(text, g13["text"])
    assert int(g13["seed"]) == R.FIXTURE_SEED and g13["latent"].shape == R.FIXTURE_LATENT
    assert tuple(g13["timesteps"]) == R.FIXTURE_TIMESTEPS and float(g13["timestep"]) == R.FIXTURE_TIMESTEP


@pytest.mark.parametrize("key", ["out", "out_t2"])
def test_oracle_matches_the_reference_forward(key):
    e64, e32 = rel_err(g13[key], _forward(key, np.float64)), rel_err(g13[key], _forward(key, np.float32))
    print(f"{key}: rel_err(fixture, ref64) {e64:.3e}, rel_err(fixture, ref32) {e32:.3e}, "
          f"rel_err(ref32, ref64) {rel_err(_forward(key, np.float32), _forward(key, np.float64)):.3e}")
    assert g13[key].shape == (2, 8, 6, 10) and np.isfinite(g13[key]).all()
    assert 1e-8 < e64 < FORWARD_BAR and e32 < FORWARD_BAR


def test_both_batch_elements_and_the_conditioning_matter():
    ref = _forward("out_t2", np.float64)
    swapped = R.forward(R.fixture_spec(), _weights(), g13["latent"], g13["timesteps"], g13["text"], np.float64, swap_conditioning=True)
    assert rel_err(swapped, ref) > 0.1
    assert rel_err(_forward("out", np.float64)[1], ref[1]) > 0.1           # element 1: timestep 500 against 37
    np.testing.assert_allclose(_forward("out", np.float64)[0], ref[0], rtol=0, atol=1e-12)


def test_host_tables_are_bit_identical_to_the_reference():
    from pygpukit_amd.diffusion.models.dit import get_2d_sincos_pos_embed, sinusoidal_embedding
    from pygpukit_amd.diffusion.ops.timestep_embed import sinusoidal_timestep_embedding_host

    for fn in (R.pos_embed_2d, lambda d, h, w: get_2d_sincos_pos_embed(d, (h, w))):
        got = fn(144, 3, 5)
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, g13["pos_embed"])
    # the grid is column-major: row 1 of the table is grid position (h=1, w=0), not (0, 1)
    np.testing.assert_array_equal(g13["pos_embed"][1, :72], R.model_sinusoidal_embedding([1.0], 72)[0])
    np.testing.assert_array_equal(g13["pos_embed"][1, 72:], R.model_sinusoidal_embedding([0.0], 72)[0])
    for fn in (R.model_sinusoidal_embedding, sinusoidal_embedding):
        np.testing.assert_array_equal(fn(g13["timesteps"], R.TIME_DIM), g13["t_sin"])
    for fn in (R.sinusoidal_timestep_embedding, sinusoidal_timestep_embedding_host):
        np.testing.assert_array_equal(fn(g13["ts_t"], 64), g13["ts_64"])
        np.testing.assert_array_equal(fn(g13["ts_t"], 10, 1000.0), g13["ts_10"])
    # the two functions differ: interleaved with divisor half_dim against [sin | cos] with half_dim - 1
    assert not np.array_equal(R.sinusoidal_timestep_embedding(g13["timesteps"], 256), g13["t_sin"])
    odd = sinusoidal_timestep_embedding_host([3.0], 9)
    assert odd.shape == (1, 9) and odd[0, 8] == 0.0


def test_oracle_ops_match_the_reference_ops():
    e = rel_err(g13["ada_out"], R.adaln(g13["ada_x"], g13["ada_scale"], g13["ada_shift"]))
    ez = rel_err(g13["ada_zero_out"], R.adaln_zero(g13["ada_x"], g13["ada_scale"], g13["ada_shift"], g13["ada_gate"], g13["ada_res"]))
    ec = rel_err(g13["ca_out"], R.attention(g13["ca_q"], g13["ca_k"], g13["ca_v"]))
    print(f"adaln {e:.3e}, adaln_zero {ez:.3e}, cross_attention {ec:.3e}")
    assert max(e, ez, ec) < OP_BAR
    # the fused form is gated_residual followed by adaln, and adaln_zero is NOT the fused form
    B, N, D = g13["ada_x"].shape
    s, y = R.fused(g13["ada_x"], g13["ada_res"], (None, g13["ada_gate"]), (None, g13["ada_scale"]), (None, g13["ada_shift"]), 1e-5)
    np.testing.assert_array_equal(y, R.adaln(s, g13["ada_scale"], g13["ada_shift"]))
    assert rel_err(y, g13["ada_zero_out"]) > 0.1


def test_padded_heads_equal_unpadded_heads_exactly():
    args = (R.fixture_spec(), _weights(), g13["latent"], g13["timesteps"], g13["text"], np.float64)
    plain = R.forward(*args, exact_sums=True)
    padded = R.forward(*args, exact_sums=True, head_width=128)
    np.testing.assert_array_equal(padded, plain)
    assert rel_err(plain, _forward("out_t2", np.float64)) < 1e-14


def test_adaln_plan_leaves_at_the_boundaries():
    from pygpukit_amd.diffusion.ops import adaln_plan

    for dtype, top, vec in (("bfloat16", 4096, 8), ("float16", 4096, 8), ("float32", 2048, 4)):
        assert adaln_plan(top, dtype) == "adaln_wave"
        assert adaln_plan(top + vec, dtype) == "adaln_block"
        assert adaln_plan(vec, dtype) == "adaln_wave"
        assert adaln_plan(vec + 1, dtype) == "adaln_block"
        assert adaln_plan(1152, dtype) == "adaln_wave"
        assert adaln_plan(1152, dtype, aligned=False) == "adaln_block"
    assert adaln_plan(100, "bfloat16") == "adaln_block" and adaln_plan(100, "float32") == "adaln_wave"
    assert adaln_plan(72, "bfloat16") == "adaln_wave" and adaln_plan(7, "float32") == "adaln_block"
    with pytest.raises(ValueError):
        adaln_plan(0, "float32")


def test_weight_packing_shapes_and_dit_plan():
    from pygpukit_amd.diffusion import PIXART_SIGMA_SPEC, PixArtSpec, dit_plan
    from pygpukit_amd.diffusion.models.dit import pack_head_columns, pack_head_rows

    w = np.arange(1, 144 * 3 + 1, dtype=np.float32).reshape(144, 3)
    rows = pack_head_rows(w, 2, 72, 128)
    assert rows.shape == (256, 3)
    np.testing.assert_array_equal(rows, R.pad_heads(w, 2, 72, 128, 0))
    np.testing.assert_array_equal(rows[:72], w[:72])
    np.testing.assert_array_equal(rows[128:200], w[72:])
    assert not rows[72:128].any() and not rows[200:].any()
    bias = pack_head_rows(np.arange(1, 145, dtype=np.float32), 2, 72, 128)
    assert bias.shape == (256,) and not bias[72:128].any() and bias[128] == 73
    cols = pack_head_columns(np.ascontiguousarray(w.T), 2, 72, 128)
    assert cols.shape == (3, 256) and cols.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(cols, R.pad_heads(w.T, 2, 72, 128, 1))
    np.testing.assert_array_equal(pack_head_rows(w, 2, 72, 72), w)

    sigma = PIXART_SIGMA_SPEC
    assert sigma.get_head_dim() == 72 and (sigma.hidden_size, sigma.num_layers, sigma.num_heads) == (1152, 28, 16)
    assert dit_plan(sigma, "bfloat16", True) == {"head_dim": 72, "head_width": 128, "padded": True, "attention": "flash"}
    assert dit_plan(sigma, "float16", False) == {"head_dim": 72, "head_width": 72, "padded": False, "attention": "fallback"}
    assert dit_plan(sigma, "float32", True) == {"head_dim": 72, "head_width": 72, "padded": False, "attention": "fallback"}
    assert dit_plan(sigma, "bfloat16", "auto")["attention"] in ("flash", "fallback")
    h64 = PixArtSpec(name="h64", hidden_size=128, num_layers=1, num_heads=2, conditioning_type="cross_attn", text_encoder_dim=32,
                     pos_embed_type="sinusoidal")
    assert dit_plan(h64, "bfloat16", False) == {"head_dim": 64, "head_width": 64, "padded": False, "attention": "flash"}
    h40 = PixArtSpec(name="h40", hidden_size=80, num_layers=1, num_heads=2, conditioning_type="cross_attn", text_encoder_dim=32,
                     pos_embed_type="sinusoidal")
    assert dit_plan(h40, "float16", True)["head_width"] == 64
    with pytest.raises(ValueError):
        dit_plan(sigma, "bfloat16", "yes")


def test_cross_attention_rejects_a_mask_before_touching_the_device():
    from pygpukit_amd.diffusion.ops import cross_attention

    with pytest.raises(NotImplementedError, match="mask"):
        cross_attention(None, None, None, 0.0, mask=object())


def test_ops_all_is_the_references_list_minus_the_vae_ops():
    from pygpukit_amd.diffusion import ops

    reference = ["group_norm", "cross_attention", "conv2d", "conv2d_transpose", "sinusoidal_timestep_embedding", "adaln", "adaln_zero"]
    kept = [n for n in reference if n not in ("group_norm", "conv2d", "conv2d_transpose")]
    assert ops.__all__[:len(kept)] == kept
    assert all(hasattr(ops, n) for n in ops.__all__)
    for n in ("group_norm", "conv2d", "conv2d_transpose"):
        assert not hasattr(ops, n) and n in ops.__doc__
