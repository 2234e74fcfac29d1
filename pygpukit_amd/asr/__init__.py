"""pygpukit_amd.asr: speech models (reference: src/pygpukit/asr).  Here: the Whisper encoder and decoder (teacher-forced
forward, KV-cache decode, generate).  WhisperModel / transcribe, the tokenizer, log-mel preprocessing (ops.audio) and checkpoint
loading are out of scope (README)."""

from pygpukit_amd.asr.whisper import (WhisperConfig, WhisperDecoder, WhisperDecoderLayer, WhisperEncoder, WhisperEncoderLayer,
                                      WhisperWeights, create_decoder, create_encoder)

__all__ = ["WhisperConfig", "WhisperWeights", "WhisperEncoder", "WhisperEncoderLayer", "create_encoder", "WhisperDecoder",
           "WhisperDecoderLayer", "create_decoder"]
