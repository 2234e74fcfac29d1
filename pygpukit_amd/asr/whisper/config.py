"""WhisperConfig: the fields, defaults and helpers of the reference's dataclass (src/pygpukit/asr/whisper/config.py), which are
Hugging Face's config.json keys.  There is no hub download here: build a config from a dict (from_dict) or a local
config.json (from_json)."""

from __future__ import annotations

import dataclasses
import json
from dataclasses import dataclass, field
from typing import Optional


@dataclass
class WhisperConfig:
    d_model: int = 1280
    encoder_layers: int = 32
    decoder_layers: int = 32
    encoder_attention_heads: int = 20
    decoder_attention_heads: int = 20
    encoder_ffn_dim: int = 5120
    decoder_ffn_dim: int = 5120
    vocab_size: int = 51866
    num_mel_bins: int = 128                  # 80 before large-v3
    max_source_positions: int = 1500         # 30 s of audio: 3000 frames, halved by the stem
    max_target_positions: int = 448
    activation_function: str = "gelu"
    dropout: float = 0.0
    attention_dropout: float = 0.0
    activation_dropout: float = 0.0
    bos_token_id: int = 50257
    eos_token_id: int = 50257
    pad_token_id: int = 50256
    decoder_start_token_id: int = 50258
    begin_suppress_tokens: list = field(default_factory=lambda: [220, 50257])
    use_cache: bool = True
    torch_dtype: str = "bfloat16"
    model_name_or_path: Optional[str] = None

    _TO_DICT = ("d_model", "encoder_layers", "decoder_layers", "encoder_attention_heads", "decoder_attention_heads",
                "encoder_ffn_dim", "decoder_ffn_dim", "vocab_size", "num_mel_bins", "max_source_positions", "max_target_positions",
                "activation_function", "dropout", "attention_dropout", "activation_dropout", "bos_token_id", "eos_token_id",
                "pad_token_id", "decoder_start_token_id")

    @classmethod
    def from_dict(cls, config_dict: dict) -> "WhisperConfig":
        """Keys that are no field are ignored; Hugging Face's "_name_or_path" becomes model_name_or_path."""
        names = {f.name for f in dataclasses.fields(cls)}
        renamed = {("model_name_or_path" if k == "_name_or_path" else k): v for k, v in config_dict.items()}
        return cls(**{k: v for k, v in renamed.items() if k in names})

    @classmethod
    def from_json(cls, json_path: str) -> "WhisperConfig":
        with open(json_path, encoding="utf-8") as f:
            return cls.from_dict(json.load(f))

    def to_dict(self) -> dict:
        return {k: getattr(self, k) for k in self._TO_DICT}

    @property
    def head_dim(self) -> int:
        return self.d_model // self.encoder_attention_heads

    @property
    def is_distilled(self) -> bool:
        return self.decoder_layers < self.encoder_layers


def _size(d_model: int, layers: int, heads: int, mels: int = 80, decoder_layers: int | None = None) -> WhisperConfig:
    return WhisperConfig(d_model=d_model, encoder_layers=layers, decoder_layers=layers if decoder_layers is None else decoder_layers,
                         encoder_attention_heads=heads, decoder_attention_heads=heads, encoder_ffn_dim=4 * d_model,
                         decoder_ffn_dim=4 * d_model, num_mel_bins=mels)


WHISPER_CONFIGS = {"tiny": _size(384, 4, 6), "base": _size(512, 6, 8), "small": _size(768, 12, 12), "medium": _size(1024, 24, 16),
                   "large": _size(1280, 32, 20), "large-v3": _size(1280, 32, 20, 128), "kotoba-v2": _size(1280, 32, 20, 128, 2)}

__all__ = ["WhisperConfig", "WHISPER_CONFIGS"]
