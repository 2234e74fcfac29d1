"""Whisper with the reference's API (src/pygpukit/asr/whisper): WhisperConfig, WhisperWeights, WhisperEncoderLayer, WhisperEncoder,
create_encoder, WhisperDecoderLayer, WhisperDecoder, create_decoder, and WhisperModel / WhisperTokenizer / TranscriptionResult /
TranscriptionSegment (model.py)."""

from pygpukit_amd.asr.whisper.config import WHISPER_CONFIGS, WhisperConfig
from pygpukit_amd.asr.whisper.decoder import WhisperDecoder, WhisperDecoderLayer, create_decoder
from pygpukit_amd.asr.whisper.encoder import WhisperEncoder, WhisperEncoderLayer, create_encoder
from pygpukit_amd.asr.whisper.loader import WhisperWeights
from pygpukit_amd.asr.whisper.model import TranscriptionResult, TranscriptionSegment, WhisperModel, WhisperTokenizer

__all__ = ["WhisperConfig", "WHISPER_CONFIGS", "WhisperWeights", "WhisperEncoder", "WhisperEncoderLayer", "create_encoder",
           "WhisperDecoder", "WhisperDecoderLayer", "create_decoder", "WhisperModel", "WhisperTokenizer", "TranscriptionResult",
           "TranscriptionSegment"]
