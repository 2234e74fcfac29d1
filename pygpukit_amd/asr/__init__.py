"""pygpukit_amd.asr: speech to text (reference: src/pygpukit/asr).  Here: Whisper preprocessing on the device (preprocessing.py:
pad_or_trim, preprocess_audio as one fused log-mel launch, over ops.audio), the Whisper encoder and decoder (teacher-forced
forward, KV-cache decode, generate) and WhisperModel with transcribe / transcribe_streaming and the tokenizer wrapper.  Checkpoint
loading, hub downloads and WhisperModel.from_pretrained are out of scope (README): build WhisperWeights.from_tensors yourself."""

from pygpukit_amd.asr.preprocessing import (WHISPER_CHUNK_LENGTH, WHISPER_HOP_LENGTH, WHISPER_N_FFT, WHISPER_N_FRAMES, WHISPER_N_MELS,
                                            WHISPER_N_SAMPLES, WHISPER_SAMPLE_RATE, normalize_mel, pad_or_trim, preprocess_audio,
                                            preprocess_audio_batch)
from pygpukit_amd.asr.whisper import (TranscriptionResult, TranscriptionSegment, WhisperConfig, WhisperDecoder, WhisperDecoderLayer,
                                      WhisperEncoder, WhisperEncoderLayer, WhisperModel, WhisperTokenizer, WhisperWeights,
                                      create_decoder, create_encoder)

__all__ = ["WhisperConfig", "WhisperWeights", "WhisperEncoder", "WhisperEncoderLayer", "create_encoder", "WhisperDecoder",
           "WhisperDecoderLayer", "create_decoder", "WhisperModel", "WhisperTokenizer", "TranscriptionResult", "TranscriptionSegment",
           "preprocess_audio", "preprocess_audio_batch", "pad_or_trim", "normalize_mel", "WHISPER_SAMPLE_RATE", "WHISPER_N_FFT",
           "WHISPER_HOP_LENGTH", "WHISPER_N_MELS", "WHISPER_CHUNK_LENGTH", "WHISPER_N_SAMPLES", "WHISPER_N_FRAMES"]
