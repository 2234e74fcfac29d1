"""WhisperModel.transcribe on the GPU, on the tiny fixture configuration (tests/whisper_decoder_ref.py) with the encoder weights of
tests/whisper_ref.py and the decoder weights of the recorded fixture, fed 4 000 samples of the audio test signal."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from tests import audio_ref as A
from tests import whisper_decoder_ref as D
from tests import whisper_ref as E

pytestmark = pytest.mark.gpu

SAMPLES = 4000
STEPS = 12


@functools.lru_cache(maxsize=None)
def _model(dtype: str):
    from pygpukit_amd.asr.whisper import WhisperModel, WhisperWeights, create_decoder, create_encoder

    cfg = D.fixture_config()
    tensors = dict(E.make_weights(cfg, E.FIXTURE_SEED))
    tensors.update(D.make_decoder_weights(cfg, D.FIXTURE_SEED))
    weights = WhisperWeights.from_tensors(cfg, tensors)
    return WhisperModel(cfg, create_encoder(cfg, weights, dtype), create_decoder(cfg, weights, dtype))


def _host(a, dtype: str) -> np.ndarray:
    h = a.to_numpy()
    return A.bf16_to_f32(h) if dtype == "bfloat16" else h.astype(np.float32)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_transcribe_equals_the_pipeline_done_by_hand(dtype, monkeypatch):
    from pygpukit_amd.asr.preprocessing import preprocess_audio

    model = _model(dtype)
    x = A.test_signal(SAMPLES)
    seen = []
    encoder_call = model.encoder.__class__.__call__
    monkeypatch.setattr(model.encoder.__class__, "__call__", lambda self, mel: (seen.append(mel), encoder_call(self, mel))[1])
    res = model.transcribe(x, max_length=STEPS)
    monkeypatch.undo()
    # what the encoder was handed: preprocess_audio's array, in the encoder's dtype, inside the oracle's bar
    assert len(seen) == 1 and seen[0].shape == (1, 16, 3001) and seen[0].dtype.name == dtype
    by_hand = preprocess_audio(x, n_mels=16, dtype=dtype)
    assert np.array_equal(seen[0].to_numpy()[0], by_hand.to_numpy())
    padded = np.zeros(480000, np.float32)
    padded[:SAMPLES] = x
    v, lo, hi = A.features_oracle(padded, fb32=A.whisper_filters(16, 400), offset=4.0, scale=0.25, dtype=dtype)
    bad = A.outside(_host(seen[0], dtype), lo, hi)
    print(f"{dtype}: mel handed to the encoder, outside {int(bad.sum())} of {bad.size}, share of the bar used {A.used(_host(seen[0], dtype), v, lo, hi):.3g}")
    assert not bad.any()
    # the tokens: decoder.generate(encoder(mel)) on the same objects
    tokens = model.decoder.generate(model.encoder(by_hand.view((1,) + by_hand.shape)), max_length=STEPS, temperature=0.0, top_k=None)
    seg = res.segments[0]
    assert seg.tokens == tokens and 1 < len(tokens) <= STEPS and tokens[0] == model.config.decoder_start_token_id
    assert (seg.start, seg.end) == (0.0, SAMPLES / 16000) and res.text == seg.text == f"<tokens: {tokens}>"


def test_48_khz_input_takes_the_resampler():
    from pygpukit_amd.ops import audio

    model = _model("float32")
    x48 = A.test_signal(3 * SAMPLES, sample_rate=48000)
    res = model.transcribe(x48, sample_rate=48000, max_length=STEPS)
    x16 = audio.resample(x48, 48000, 16000)
    assert x16.shape == (SAMPLES,)
    same = model.transcribe(x16.to_numpy(), max_length=STEPS)
    assert len(res.segments) == 1 and res.segments[0].end == SAMPLES / 16000 and 1 < len(res.segments[0].tokens) <= STEPS
    assert res.segments[0].tokens == same.segments[0].tokens


def test_streaming_runs_each_chunk_through_the_device():
    model = _model("float32")
    x = A.test_signal(SAMPLES)
    segs = list(model.transcribe_streaming(x, chunk_length=0.125, overlap=0.0, max_length=6))
    assert [(s.start, s.end) for s in segs] == [(0.0, 0.125), (0.125, 0.25)] and all(1 < len(s.tokens) <= 6 for s in segs)
    assert segs[0].tokens == model.transcribe(x[:2000], max_length=6).segments[0].tokens
