"""WhisperModel: samples -> text (reference: src/pygpukit/asr/whisper/model.py).  Same signatures and timing arithmetic, with one
change: the reference computes the mel features on the host, in a Python loop over 3001 frames, and uploads them; here
preprocessing is one launch on the device (asr/preprocessing.py) and hands the encoder an array of the encoder's own dtype.  The
decoder runs its cached fused path (set_encoder_states + generate)."""

from __future__ import annotations

import os
from collections.abc import Iterator
from dataclasses import dataclass, field

import numpy as np

from pygpukit_amd.asr.preprocessing import (WHISPER_CHUNK_LENGTH, WHISPER_SAMPLE_RATE, load_audio, preprocess_audio)
from pygpukit_amd.asr.whisper.config import WhisperConfig
from pygpukit_amd.asr.whisper.decoder import WhisperDecoder
from pygpukit_amd.asr.whisper.encoder import WhisperEncoder
from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.ops import audio as audio_ops


@dataclass
class TranscriptionSegment:
    """A single transcription segment with timing information."""

    text: str
    start: float  # seconds
    end: float  # seconds
    tokens: list[int] = field(default_factory=list)


@dataclass
class TranscriptionResult:
    """Complete transcription result."""

    text: str
    segments: list[TranscriptionSegment] = field(default_factory=list)
    language: str | None = None


class WhisperTokenizer:
    """tokenizer.json of a model directory through the HuggingFace `tokenizers` library; without the library or the file, encode
    and decode raise and WhisperModel falls back to "<tokens: [...]>"."""

    def __init__(self, model_path: str):
        self.model_path = model_path
        self._tokenizer = None
        self._load_tokenizer()

    def _load_tokenizer(self) -> None:
        try:
            from tokenizers import Tokenizer
        except ImportError:
            return
        path = os.path.join(self.model_path, "tokenizer.json")
        if os.path.exists(path):
            self._tokenizer = Tokenizer.from_file(path)

    @property
    def available(self) -> bool:
        return self._tokenizer is not None

    def encode(self, text: str) -> list[int]:
        if self._tokenizer is None:
            raise RuntimeError("Tokenizer not available")
        return self._tokenizer.encode(text).ids

    def decode(self, token_ids: list[int], skip_special_tokens: bool = True) -> str:
        if self._tokenizer is None:
            raise RuntimeError("Tokenizer not available")
        return self._tokenizer.decode(list(token_ids), skip_special_tokens=skip_special_tokens)


class WhisperModel:
    """model = WhisperModel(config, create_encoder(config, weights, dtype), create_decoder(config, weights, dtype), tokenizer)
    result = model.transcribe(samples, sample_rate=48000)
    for segment in model.transcribe_streaming(samples, chunk_length=30, overlap=1.0): ..."""

    def __init__(self, config: WhisperConfig, encoder: WhisperEncoder, decoder: WhisperDecoder, tokenizer: WhisperTokenizer | None = None):
        self.config = config
        self.encoder = encoder
        self.decoder = decoder
        self.tokenizer = tokenizer

    @classmethod
    def from_pretrained(cls, model_path_or_id: str, cache_dir: str | None = None) -> "WhisperModel":
        raise NotImplementedError(
            "WhisperModel.from_pretrained: checkpoint loading and hub downloads are out of scope. Read the tensors yourself, build "
            "WhisperWeights.from_tensors(tensors, config), then WhisperModel(config, create_encoder(config, weights), "
            "create_decoder(config, weights), WhisperTokenizer(model_dir)).")

    def transcribe(self, audio: "np.ndarray | GPUArray | str", sample_rate: int | None = None, language: str | None = None,
                   max_length: int = 448, temperature: float = 0.0, **kwargs) -> TranscriptionResult:
        """One chunk (padded or trimmed to 30 s) -> TranscriptionResult with one segment spanning the input.  sample_rate other
        than 16000 goes through the device resampler; the segment's end is the resampled length / 16000, as in the reference."""
        if isinstance(audio, str):
            audio, sample_rate = load_audio(audio)
        if sample_rate is not None and sample_rate != WHISPER_SAMPLE_RATE:
            audio = audio_ops.resample(audio, sample_rate, WHISPER_SAMPLE_RATE)
        n_samples = audio.size if isinstance(audio, GPUArray) else len(audio)
        tokens = self._transcribe_chunk(audio, max_length, temperature)
        text = self._decode_tokens(tokens)
        segment = TranscriptionSegment(text=text, start=0.0, end=n_samples / WHISPER_SAMPLE_RATE, tokens=tokens)
        return TranscriptionResult(text=text, segments=[segment], language=language)

    def transcribe_streaming(self, audio: np.ndarray, language: str | None = None, chunk_length: float = WHISPER_CHUNK_LENGTH,
                             overlap: float = 0.0, max_length: int = 448, temperature: float = 0.0, **kwargs) -> Iterator[TranscriptionSegment]:
        """16 kHz samples in chunks of chunk_length seconds that start chunk_length - overlap apart; one segment per chunk."""
        samples_per_chunk = int(chunk_length * WHISPER_SAMPLE_RATE)
        stride = samples_per_chunk - int(overlap * WHISPER_SAMPLE_RATE)
        if samples_per_chunk < 1 or stride < 1:
            raise ValueError(f"transcribe_streaming: needs chunk_length > overlap >= 0, got {chunk_length} and {overlap}")
        start_sample = 0
        while start_sample < len(audio):
            end_sample = min(start_sample + samples_per_chunk, len(audio))
            tokens = self._transcribe_chunk(audio[start_sample:end_sample], max_length, temperature)
            yield TranscriptionSegment(text=self._decode_tokens(tokens), start=start_sample / WHISPER_SAMPLE_RATE,
                                       end=end_sample / WHISPER_SAMPLE_RATE, tokens=tokens)
            start_sample += stride

    def _transcribe_chunk(self, samples, max_length: int, temperature: float) -> list[int]:
        encoder_output = self.encoder(self._preprocess_audio(samples))
        return self.decoder.generate(encoder_output, max_length=max_length, temperature=temperature,
                                     top_k=None if temperature == 0.0 else 50)

    def _preprocess_audio(self, samples) -> GPUArray:
        """16 kHz samples -> [1, n_mels, 3001] in the encoder's dtype: one launch, no host round trip."""
        mel = preprocess_audio(samples, n_mels=self.config.num_mel_bins, dtype=getattr(self.encoder, "dtype", "float32"))
        return mel.view((1,) + mel.shape)

    def _decode_tokens(self, tokens: list[int]) -> str:
        if self.tokenizer is not None and getattr(self.tokenizer, "available", True):
            return self.tokenizer.decode(tokens, skip_special_tokens=True)
        return f"<tokens: {tokens}>"


__all__ = ["WhisperModel", "WhisperTokenizer", "TranscriptionResult", "TranscriptionSegment"]
