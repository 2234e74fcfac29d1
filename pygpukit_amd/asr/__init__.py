"""pygpukit_amd.asr: speech models (reference: src/pygpukit/asr).  Here: the Whisper ENCODER.  The decoder, generate / transcribe,
log-mel preprocessing (ops.audio) and checkpoint loading are out of scope (README)."""

from pygpukit_amd.asr.whisper import WhisperConfig, WhisperEncoder, WhisperEncoderLayer, WhisperWeights, create_encoder

__all__ = ["WhisperConfig", "WhisperWeights", "WhisperEncoder", "WhisperEncoderLayer", "create_encoder"]
