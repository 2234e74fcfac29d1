"""WhisperWeights: host (NumPy) weights under the reference's attribute names (src/pygpukit/asr/whisper/loader.py), filled from a
name -> ndarray dict with Hugging Face's tensor names.  Encoder:

    model.encoder.conv1.{weight,bias}   model.encoder.conv2.{weight,bias}   model.encoder.embed_positions.weight
    model.encoder.layers.{i}.self_attn.{q,k,v,out}_proj.{weight,bias}       (k_proj has no bias in Whisper: None)
    model.encoder.layers.{i}.self_attn_layer_norm.{weight,bias}
    model.encoder.layers.{i}.fc1.{weight,bias}   model.encoder.layers.{i}.fc2.{weight,bias}
    model.encoder.layers.{i}.final_layer_norm.{weight,bias}                 model.encoder.layer_norm.{weight,bias}

Decoder, filled when the dict holds model.decoder.embed_tokens.weight (otherwise its attributes stay None / []):

    model.decoder.embed_tokens.weight   model.decoder.embed_positions.weight   model.decoder.layer_norm.{weight,bias}
    model.decoder.layers.{i}.self_attn.* and self_attn_layer_norm.*      as the encoder's
    model.decoder.layers.{i}.encoder_attn.{q,k,v,out}_proj.{weight,bias}    -> cross_attn_* (k_proj has no bias: None)
    model.decoder.layers.{i}.encoder_attn_layer_norm.{weight,bias}          -> cross_attn_layer_norm_*
    model.decoder.layers.{i}.fc1 / fc2 / final_layer_norm
    proj_out.weight                                                         absent: tied to embed_tokens

Reading real checkpoints (safetensors files, hub downloads) is out of scope."""

from __future__ import annotations

from typing import Optional

import numpy as np

from pygpukit_amd.asr.whisper.config import WhisperConfig

_LAYER_KEYS = {"self_attn_q_weight": "self_attn.q_proj.weight", "self_attn_q_bias": "self_attn.q_proj.bias",
               "self_attn_k_weight": "self_attn.k_proj.weight", "self_attn_k_bias": "self_attn.k_proj.bias",
               "self_attn_v_weight": "self_attn.v_proj.weight", "self_attn_v_bias": "self_attn.v_proj.bias",
               "self_attn_out_weight": "self_attn.out_proj.weight", "self_attn_out_bias": "self_attn.out_proj.bias",
               "self_attn_layer_norm_weight": "self_attn_layer_norm.weight", "self_attn_layer_norm_bias": "self_attn_layer_norm.bias",
               "fc1_weight": "fc1.weight", "fc1_bias": "fc1.bias", "fc2_weight": "fc2.weight", "fc2_bias": "fc2.bias",
               "final_layer_norm_weight": "final_layer_norm.weight", "final_layer_norm_bias": "final_layer_norm.bias"}
_OPTIONAL = ("self_attn_k_bias", "cross_attn_k_bias")
# the reference's 26 decoder-layer keys: the encoder's 16 plus cross attention (Hugging Face's encoder_attn)
_DECODER_LAYER_KEYS = {**{k: v for k, v in _LAYER_KEYS.items() if k.startswith("self_attn")},
                       **{"cross" + k[4:]: "encoder" + v[4:] for k, v in _LAYER_KEYS.items() if k.startswith("self_attn")},
                       **{k: v for k, v in _LAYER_KEYS.items() if not k.startswith("self_attn")}}
_DECODER_MARK = "model.decoder.embed_tokens.weight"


class WhisperWeights:
    def __init__(self, config: WhisperConfig):
        self.config = config
        self.encoder_conv1_weight: Optional[np.ndarray] = None
        self.encoder_conv1_bias: Optional[np.ndarray] = None
        self.encoder_conv2_weight: Optional[np.ndarray] = None
        self.encoder_conv2_bias: Optional[np.ndarray] = None
        self.encoder_embed_positions: Optional[np.ndarray] = None
        self.encoder_layers: list = []               # one dict per layer, keys of _LAYER_KEYS
        self.encoder_layer_norm_weight: Optional[np.ndarray] = None
        self.encoder_layer_norm_bias: Optional[np.ndarray] = None
        self.decoder_embed_tokens: Optional[np.ndarray] = None
        self.decoder_embed_positions: Optional[np.ndarray] = None
        self.decoder_layers: list = []               # one dict per layer, keys of _DECODER_LAYER_KEYS
        self.decoder_layer_norm_weight: Optional[np.ndarray] = None
        self.decoder_layer_norm_bias: Optional[np.ndarray] = None
        self.proj_out_weight: Optional[np.ndarray] = None

    @classmethod
    def from_tensors(cls, config: WhisperConfig, tensors: dict) -> "WhisperWeights":
        """`tensors`: Hugging Face name -> ndarray.  A missing tensor raises KeyError naming it, except k_proj.bias.  A dict with
        decoder tensors only (not one model.encoder.* name) fills the decoder side alone; with any encoder tensor present the
        whole encoder is required."""
        w = cls(config)
        if _DECODER_MARK in tensors:
            w._load_decoder(tensors)
            if not any(name.startswith("model.encoder.") for name in tensors):
                return w
        enc = "model.encoder."
        for attr, name in (("encoder_conv1_weight", "conv1.weight"), ("encoder_conv1_bias", "conv1.bias"),
                           ("encoder_conv2_weight", "conv2.weight"), ("encoder_conv2_bias", "conv2.bias"),
                           ("encoder_embed_positions", "embed_positions.weight"), ("encoder_layer_norm_weight", "layer_norm.weight"),
                           ("encoder_layer_norm_bias", "layer_norm.bias")):
            setattr(w, attr, np.asarray(tensors[enc + name]))
        for i in range(config.encoder_layers):
            layer = {}
            for key, name in _LAYER_KEYS.items():
                full = f"{enc}layers.{i}.{name}"
                layer[key] = np.asarray(tensors[full]) if (key not in _OPTIONAL or full in tensors) else None
            w.encoder_layers.append(layer)
        return w

    def _load_decoder(self, tensors: dict) -> None:
        dec = "model.decoder."
        for attr, name in (("decoder_embed_tokens", "embed_tokens.weight"), ("decoder_embed_positions", "embed_positions.weight"),
                           ("decoder_layer_norm_weight", "layer_norm.weight"), ("decoder_layer_norm_bias", "layer_norm.bias")):
            setattr(self, attr, np.asarray(tensors[dec + name]))
        self.proj_out_weight = np.asarray(tensors["proj_out.weight"]) if "proj_out.weight" in tensors else self.decoder_embed_tokens
        for i in range(self.config.decoder_layers):
            layer = {}
            for key, name in _DECODER_LAYER_KEYS.items():
                full = f"{dec}layers.{i}.{name}"
                layer[key] = np.asarray(tensors[full]) if (key not in _OPTIONAL or full in tensors) else None
            self.decoder_layers.append(layer)


__all__ = ["WhisperWeights"]
