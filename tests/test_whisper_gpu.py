"""WhisperEncoder on the GPU, on the configuration of tests/golden/g10_whisper.npz (d_model 128, 2 layers, 2 heads of 64, 16 mel
bins, 74 frames -> 37 positions), against the reference's recorded float32 output and the float64 oracle of tests/whisper_ref.py.

bfloat16 / float16: rel_err <= 1e-2 on the final hidden states, the oracle running on weights and mel rounded to the dtype.

float32: the yardstick is the reference's own distance from exact arithmetic, rel_err(fixture, ref64) = 4.25e-7 - a property of
the reference's float32 CPU path and of the oracle, nothing of the code under test.  The bar is FACTOR32 times that distance,
FACTOR32 the smallest power of two at least twice the worst measured ratio rel_err(gpu, ref64) / rel_err(fixture, ref64), and
never more than 1e-4.  Measured on an MI355X: rel_err(gpu, ref64) = 4.277e-7, ratio 1.007, on the fixture's mel and 4.259e-7, ratio
1.003, on the second element of the batch test; twice the worst is 2.014, hence FACTOR32 = 4 and a bar of 1.70e-6."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from tests import whisper_ref as R
from tests.conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

g10 = load_golden("g10_whisper.npz")
FACTOR32 = 4.0
CAP32 = 1e-4


def _pk(dtype):
    from pygpukit_amd.core.dtypes import bfloat16, float16, float32

    return {"f32": float32, "bf16": bfloat16, "f16": float16}[dtype]


def _host(a, dtype):
    h = a.to_numpy()
    return R.from_words(h if dtype == "f32" or h.dtype == np.uint16 else h.view(np.uint16), dtype).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _tensors():
    return R.make_weights(R.fixture_config(), int(g10["enc_seed"]))


@functools.lru_cache(maxsize=None)
def _encoder(dtype):
    from pygpukit_amd.asr.whisper import WhisperWeights, create_encoder

    cfg = R.fixture_config()
    return create_encoder(cfg, WhisperWeights.from_tensors(cfg, _tensors()), dtype=_pk(dtype))


@functools.lru_cache(maxsize=None)
def _ref64(dtype):
    out = R.encoder_forward(R.fixture_config(), _tensors(), g10["enc_mel"], np.float64, round_dtype=dtype)
    out.setflags(write=False)
    return out


def _mel(mel, dtype):
    from pygpukit_amd.core import from_numpy

    w = R.to_words(mel, dtype)
    return from_numpy(np.ascontiguousarray(w.view(np.float16) if dtype == "f16" else w))


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_encoder_16bit_against_the_oracle(dtype):
    out = _encoder(dtype)(_mel(g10["enc_mel"], dtype))
    assert out.shape == (1, 37, 128) and out.dtype == _pk(dtype)
    got = _host(out, dtype)
    e, e_fix = rel_err(got, _ref64(dtype)), rel_err(got, g10["enc_out"])
    print(f"WhisperEncoder {dtype}: rel_err vs ref64 {e:.3e}, vs the reference's float32 fixture {e_fix:.3e}")
    assert np.isfinite(got).all() and e <= 1e-2


def test_encoder_float32_against_the_reference_and_the_oracle():
    yard = rel_err(g10["enc_out"], _ref64("f32"))
    bar = FACTOR32 * yard
    assert 1e-7 < yard < 1e-6 and bar <= CAP32
    out = _encoder("f32")(_mel(g10["enc_mel"], "f32"))
    assert out.shape == (1, 37, 128) and out.dtype == _pk("f32")
    got = _host(out, "f32")
    e = rel_err(got, _ref64("f32"))
    print(f"WhisperEncoder f32: rel_err(gpu, ref64) {e:.3e}, rel_err(fixture, ref64) {yard:.3e}, ratio {e / yard:.3f}, "
          f"rel_err(gpu, fixture) {rel_err(got, g10['enc_out']):.3e}")
    assert e <= bar


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_batch_of_two_equals_two_single_calls_bit_for_bit(dtype):
    cfg = R.fixture_config()
    mel = np.concatenate([g10["enc_mel"], R.make_mel(cfg, R.FIXTURE_FRAMES, 4242)])
    enc = _encoder(dtype)
    both = enc(_mel(mel, dtype)).to_numpy()
    assert both.shape == (2, 37, 128)
    for b in range(2):
        np.testing.assert_array_equal(both[b:b + 1], enc(_mel(mel[b:b + 1], dtype)).to_numpy())
    if dtype == "f32":
        ref = R.encoder_forward(cfg, _tensors(), mel[1:], np.float64)
        e, yard = rel_err(both[1:], ref), rel_err(g10["enc_out"], _ref64("f32"))
        print(f"WhisperEncoder f32 batch element 1: rel_err(gpu, ref64) {e:.3e}, ratio {e / yard:.3f}")
        assert e <= FACTOR32 * yard


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_longer_mel_is_clamped_to_max_source_positions(dtype):
    """90 frames -> 45 stem positions > max_source_positions = 37: the first 37 are kept, as in the reference, and they are
    not the encoding of the first 74 frames alone (position 36 sees frame 74 through both convolutions)."""
    cfg = R.fixture_config()
    mel = R.make_mel(cfg, 90, 777)
    out = _encoder(dtype)(_mel(mel, dtype))
    assert out.shape == (1, cfg.max_source_positions, cfg.d_model)
    ref = R.encoder_forward(cfg, _tensors(), mel, np.float64, round_dtype=dtype)
    assert ref.shape == out.shape
    e = rel_err(_host(out, dtype), ref)
    assert e <= (1e-2 if dtype == "bf16" else FACTOR32 * rel_err(g10["enc_out"], _ref64("f32")))
    assert rel_err(R.encoder_forward(cfg, _tensors(), mel[:, :, :74], np.float64, round_dtype=dtype), ref) > 2e-2


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_the_stem_is_two_launches(dtype):
    """Captured into a graph, the stem with pre-packed weights is exactly two kernel nodes: conv + GELU, and conv + GELU +
    channels-last store + position add."""
    import pygpukit_amd as pk

    enc = _encoder(dtype)
    mel = _mel(g10["enc_mel"], dtype)
    eager = enc._conv_stem(mel).to_numpy()          # also builds the cached position rows outside the capture
    graph = pk.CudaGraph()
    graph.begin_capture()
    x = enc._conv_stem(mel)
    graph.end_capture()
    assert graph.is_ready() and graph.num_nodes == 2
    graph.replay()
    graph.synchronize()
    np.testing.assert_array_equal(x.to_numpy(), eager)
