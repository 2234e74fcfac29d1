"""VAE.decode on the GPU against the float64 decoder of tests/vae_ref.py on the fixture configuration: block_out_channels
(16, 32, 32), one layer per block, 4 groups, latent [2, 4, 5, 7] -> image [2, 3, 20, 28] - a shortcut convolution, two upsamples
and the mid-block attention on 35 tokens.

float32: rel_err(decode, ref64) <= FACTOR32 * rel_err(ref32, ref64), ref32 the oracle run in np.float32 on the same inputs; never
above 1e-4.  FACTOR32 is the smallest power of two at least twice the worst measured ratio (MEASURED32).

16-bit: the project's rel_err <= 1e-2 does not fit a 20-op chain.  The oracle with every op's output rounded to the dtype sits at
`floor` from the same oracle with exact activations (same rounded weights and latent); that distance belongs to the dtype and the
fixture.  The bar is FACTOR16 * floor against the exact-activation oracle, FACTOR16 the smallest power of two at least twice the
measured ratio (MEASURED16) - the margin covers the fp32 the device keeps inside a fused op where the restatement rounds, and
another summation order.  Condition: FACTOR16 <= 4; a ratio above 2 means an op loses precision it should keep."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from tests import vae_ref as R

pytestmark = pytest.mark.gpu

MEASURED32 = 2.174      # worst rel_err(gpu, ref64) / rel_err(ref32, ref64), measured on an MI355X (sdpa path without
                        # post_quant_conv; the other float32 cases 1.913 - 2.059); twice it is 4.348
FACTOR32 = 8.0
MEASURED16 = 1.043      # worst rel_err(gpu, exact) / floor, measured on an MI355X (float16 sdpa; float16 matmul 0.971,
                        # bfloat16 0.994 and 0.952); twice it is 2.086
FACTOR16 = 4.0
SHIFT = 0.25
PATHS = ("sdpa", "matmul")


@functools.lru_cache(maxsize=None)
def _oracle(post_quant, shift, latent_scale, round_dtype, mode):
    """mode: "f64" | "f32" | "rounded" (every op's output rounded to round_dtype)"""
    spec = R.fixture_spec(shift)
    weights = R.make_weights(spec, R.FIXTURE_SEED, post_quant)
    latent = R.make_latent(R.FIXTURE_SEED) * np.float32(latent_scale)
    out = R.forward(spec, weights, latent, np.float32 if mode == "f32" else np.float64, round_dtype, mode == "rounded")
    out.setflags(write=False)
    return out


def _decode(dtype, path, post_quant=True, shift=0.0, latent_scale=1.0):
    from pygpukit_amd.core import from_numpy
    from pygpukit_amd.core.dtypes import as_dtype, float32
    from pygpukit_amd.diffusion import VAE, vae_plan

    spec = R.fixture_spec(shift)
    vae = VAE(spec, R.make_weights(spec, R.FIXTURE_SEED, post_quant), dtype=dtype, attention=path)
    assert vae_plan(spec, dtype, (5, 7), path, post_quant, 2)["attention"] == path
    latent = from_numpy(R.make_latent(R.FIXTURE_SEED) * np.float32(latent_scale)).astype(as_dtype(dtype))
    out = vae.decode(latent)
    assert out.shape == (2, 3, 20, 28) and out.dtype == as_dtype(dtype)
    return out.astype(float32).to_numpy().astype(np.float64)


def _check32(name, got, **kw):
    ref64, ref32 = _oracle(round_dtype=None, mode="f64", **kw), _oracle(round_dtype=None, mode="f32", **kw)
    yard, err = R.rel_err(ref32, ref64), R.rel_err(got, ref64)
    print(f"{name}: rel_err {err:.3e}, rel_err(ref32, ref64) {yard:.3e}, ratio {err / yard:.3f}")
    assert np.isfinite(got).all() and np.abs(got).max() <= 1.0
    assert err <= min(FACTOR32 * yard, 1e-4), f"{name}: rel_err {err:.3e} over {FACTOR32} x {yard:.3e}"
    return ref64


@pytest.mark.parametrize("path", PATHS)
def test_decode_float32(path):
    kw = dict(post_quant=True, shift=0.0, latent_scale=1.0)
    _check32(f"decode float32 {path}", _decode("float32", path), **kw)


@pytest.mark.parametrize("path", PATHS)
def test_decode_float32_without_post_quant_conv(path):
    _check32(f"decode float32 {path} no post_quant_conv", _decode("float32", path, post_quant=False), post_quant=False, shift=0.0, latent_scale=1.0)


def test_decode_float32_with_a_shift_factor():
    ref = _check32("decode float32 shift_factor", _decode("float32", "matmul", shift=SHIFT), post_quant=True, shift=SHIFT, latent_scale=1.0)
    assert R.rel_err(ref, _oracle(True, 0.0, 1.0, None, "f64")) > 1e-2             # the shift matters on this fixture


def test_decode_float32_clamps():
    got = _decode("float32", "sdpa", latent_scale=4.0)
    ref = _check32("decode float32 latent x 4", got, post_quant=True, shift=0.0, latent_scale=4.0)
    clamped = np.abs(ref) == 1.0
    assert clamped.mean() > 0.05 and np.array_equal(np.abs(got)[clamped], np.ones(int(clamped.sum())))


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("dtype", ("bfloat16", "float16"))
def test_decode_16bit(dtype, path):
    assert FACTOR16 <= 4
    kw = dict(post_quant=True, shift=0.0, latent_scale=1.0, round_dtype=dtype)
    exact, rounded = _oracle(mode="f64", **kw), _oracle(mode="rounded", **kw)
    floor = R.rel_err(rounded, exact)
    got = _decode(dtype, path)
    err = R.rel_err(got, exact)
    print(f"decode {dtype} {path}: rel_err {err:.3e}, floor {floor:.3e}, ratio {err / floor:.3f}")
    assert np.isfinite(got).all() and err <= FACTOR16 * floor, f"decode {dtype} {path}: rel_err {err:.3e} over {FACTOR16} x floor {floor:.3e}"


def test_decode_is_deterministic_and_encode_is_not_built():
    from pygpukit_amd.diffusion import VAE

    a, b = _decode("bfloat16", "matmul"), _decode("bfloat16", "matmul")
    assert np.array_equal(a, b)
    spec = R.fixture_spec()
    with pytest.raises(NotImplementedError):
        VAE(spec, R.make_weights(spec, R.FIXTURE_SEED)).encode(None)


def test_from_safetensors_decodes_like_the_weights_it_was_written_from(tmp_path):
    from pygpukit_amd.core import from_numpy
    from pygpukit_amd.diffusion import VAE
    from pygpukit_amd.llm.safetensors import save_safetensors

    spec = R.fixture_spec()
    w = R.make_weights(spec, R.FIXTURE_SEED)
    tensors = {k: (v, "F32") for k, v in w.items()}
    tensors["encoder.conv_in.weight"] = (np.ones((4, 3, 3, 3), np.float32), "F32")
    save_safetensors(str(tmp_path / "vae.safetensors"), tensors)
    vae = VAE.from_safetensors(tmp_path, spec, dtype="float32", attention="matmul")
    got = vae.decode(from_numpy(R.make_latent(R.FIXTURE_SEED))).to_numpy().astype(np.float64)
    assert np.array_equal(got, _decode("float32", "matmul"))
    with pytest.raises(ValueError, match="the spec needs"):                            # no spec: 4 latent channels -> the SDXL spec,
        VAE.from_safetensors(tmp_path / "vae.safetensors")                             # whose shapes these weights do not have
