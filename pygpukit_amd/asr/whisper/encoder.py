"""Whisper encoder (reference: src/pygpukit/asr/whisper/encoder.py): conv stem, position embedding, pre-norm transformer layers
with bidirectional attention, final layer norm.  mel [B, n_mels, n_frames] -> [B, seq, d_model], seq = (n_frames + 1) // 2
clamped to max_source_positions as in the reference.

What runs here, against the reference's op sequence:
  * stem: TWO conv1d launches (weights packed once at construction).  The first fuses bias + GELU; the second (stride 2) fuses
    bias + GELU, writes [B, seq, d_model] directly and adds embed_positions[:seq] - the reference runs conv, gelu, conv, gelu, a
    transpose and a broadcast add;
  * per batch element and layer: layernorm, ONE q/k/v GEMM on the [3 d_model, d_model] weight concatenated at construction
    (k_proj has no bias: zeros), sdpa_noncausal_strided reading the [seq, 3 d_model] projection in place - the reference
    materialises the [H, seq, seq] scores between two batched matmuls and transposes four times -, out_proj, residual add,
    layernorm, fc1 through linear_bias_gelu, fc2, residual add.
`dtype`: float32 (the reference's), bfloat16 or float16; head_dim 64 (every Whisper size) takes the MFMA flash kernel in the
16-bit dtypes."""

from __future__ import annotations

import numpy as np

from pygpukit_amd.asr.whisper.config import WhisperConfig
from pygpukit_amd.asr.whisper.loader import WhisperWeights
from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import DataType, as_dtype, float32
from pygpukit_amd.core.factory import from_numpy
from pygpukit_amd.ops.conv import conv1d, conv1d_pack_weight
from pygpukit_amd.ops.elementwise import add
from pygpukit_amd.ops.matmul import linear_bias_gelu, matmul_nt
from pygpukit_amd.ops.nn.attention import sdpa_noncausal_strided
from pygpukit_amd.ops.nn.norm import layernorm


def _to_gpu(arr, dtype: DataType) -> GPUArray:
    return from_numpy(np.ascontiguousarray(arr, dtype=np.float32)).astype(dtype)


class WhisperEncoderLayer:
    """x = x + attention(layer_norm(x)); x = x + ffn(layer_norm(x)) on one batch element's [seq, d_model] rows."""

    def __init__(self, config: WhisperConfig, layer_weights: dict, dtype: "str | DataType" = float32):
        self.config = config
        self.dtype = as_dtype(dtype)
        self.d_model = config.d_model
        self.n_heads = config.encoder_attention_heads
        self.head_dim = config.d_model // config.encoder_attention_heads
        w = layer_weights
        k_bias = w["self_attn_k_bias"] if w.get("self_attn_k_bias") is not None else np.zeros(self.d_model, np.float32)
        self.qkv_weight = _to_gpu(np.concatenate([w["self_attn_q_weight"], w["self_attn_k_weight"], w["self_attn_v_weight"]], axis=0), self.dtype)
        self.qkv_bias = _to_gpu(np.concatenate([w["self_attn_q_bias"], k_bias, w["self_attn_v_bias"]]), self.dtype)
        for name, key in (("out_weight", "self_attn_out_weight"), ("out_bias", "self_attn_out_bias"),
                          ("attn_ln_weight", "self_attn_layer_norm_weight"), ("attn_ln_bias", "self_attn_layer_norm_bias"),
                          ("fc1_weight", "fc1_weight"), ("fc1_bias", "fc1_bias"), ("fc2_weight", "fc2_weight"), ("fc2_bias", "fc2_bias"),
                          ("ffn_ln_weight", "final_layer_norm_weight"), ("ffn_ln_bias", "final_layer_norm_bias")):
            setattr(self, name, _to_gpu(w[key], self.dtype))

    def __call__(self, x: GPUArray) -> GPUArray:
        if x.ndim != 2 or x.shape[1] != self.d_model:
            raise ValueError(f"WhisperEncoderLayer: x must be [seq, {self.d_model}], got {x.shape}")
        x = add(x, self._self_attention(layernorm(x, self.attn_ln_weight, self.attn_ln_bias)))
        return add(x, self._ffn(layernorm(x, self.ffn_ln_weight, self.ffn_ln_bias)))

    def _self_attention(self, h: GPUArray) -> GPUArray:
        seq, d, hd = h.shape[0], self.d_model, self.head_dim
        qkv = matmul_nt(h, self.qkv_weight, self.qkv_bias)                        # [seq, 3 d]: q | k | v per row
        rest = qkv.size - 2 * d
        k, v = qkv._view(d, (rest,)), qkv._view(2 * d, (rest,))
        attn = GPUArray((seq, d), h.dtype)
        sdpa_noncausal_strided(qkv, k, v, attn, self.n_heads, self.n_heads, seq, seq, hd, (hd, 3 * d), (hd, 3 * d), (hd, d))
        return matmul_nt(attn, self.out_weight, self.out_bias)

    def _ffn(self, h: GPUArray) -> GPUArray:
        return matmul_nt(linear_bias_gelu(h, self.fc1_weight, self.fc1_bias), self.fc2_weight, self.fc2_bias)


class WhisperEncoder:
    def __init__(self, config: WhisperConfig, weights: WhisperWeights, dtype: "str | DataType" = float32):
        self.config = config
        self.dtype = as_dtype(dtype)
        self.d_model = config.d_model
        self.n_layers = config.encoder_layers
        if config.d_model % config.encoder_attention_heads:
            raise ValueError(f"WhisperEncoder: d_model {config.d_model} is no multiple of {config.encoder_attention_heads} heads")
        self.conv1_weight, self.conv1_bias = _to_gpu(weights.encoder_conv1_weight, self.dtype), _to_gpu(weights.encoder_conv1_bias, self.dtype)
        self.conv2_weight, self.conv2_bias = _to_gpu(weights.encoder_conv2_weight, self.dtype), _to_gpu(weights.encoder_conv2_bias, self.dtype)
        packed = self.dtype != float32
        self.conv1_packed = conv1d_pack_weight(self.conv1_weight) if packed else None
        self.conv2_packed = conv1d_pack_weight(self.conv2_weight) if packed else None
        self._positions = np.ascontiguousarray(weights.encoder_embed_positions, dtype=np.float32)
        self.embed_positions = _to_gpu(self._positions, self.dtype)
        self._pos_rows: dict[int, GPUArray] = {}
        self.layer_norm_weight = _to_gpu(weights.encoder_layer_norm_weight, self.dtype)
        self.layer_norm_bias = _to_gpu(weights.encoder_layer_norm_bias, self.dtype)
        self.layers = [WhisperEncoderLayer(config, lw, self.dtype) for lw in weights.encoder_layers]

    def _position_rows(self, rows: int) -> GPUArray:
        """embed_positions as the `add` operand of the second conv: its first `rows` rows; zero rows beyond max_source_positions
        (those outputs are dropped by the clamp)."""
        if rows not in self._pos_rows:
            pos = np.zeros((rows, self.d_model), np.float32)
            n = min(rows, self._positions.shape[0])
            pos[:n] = self._positions[:n]
            self._pos_rows[rows] = _to_gpu(pos, self.dtype)
        return self._pos_rows[rows]

    def _conv_stem(self, mel: GPUArray) -> GPUArray:
        """[B, n_mels, n_frames] -> [B, (n_frames + 1) // 2, d_model], position embedding added: two launches."""
        x = conv1d(mel, self.conv1_weight, self.conv1_bias, padding=1, activation="gelu", packed_weight=self.conv1_packed)
        rows = (x.shape[2] - 1) // 2 + 1
        return conv1d(x, self.conv2_weight, self.conv2_bias, stride=2, padding=1, activation="gelu", channels_last_out=True,
                      add=self._position_rows(rows), packed_weight=self.conv2_packed)

    def __call__(self, mel: GPUArray) -> GPUArray:
        if mel.ndim != 3 or mel.shape[1] != self.config.num_mel_bins:
            raise ValueError(f"WhisperEncoder: mel must be [batch, {self.config.num_mel_bins}, n_frames], got {mel.shape}")
        x = self._conv_stem(mel.astype(self.dtype))
        batch, rows, d = x.shape
        seq = min(rows, self.embed_positions.shape[0])          # the reference's clamp to max_source_positions
        out = GPUArray((batch, seq, d), self.dtype)
        for b in range(batch):
            h = x._view(b * rows * d, (seq, d))
            for layer in self.layers:
                h = layer(h)
            layernorm(h, self.layer_norm_weight, self.layer_norm_bias, out=out._view(b * seq * d, (seq, d)))
        return out


def create_encoder(config: WhisperConfig, weights: WhisperWeights, dtype: "str | DataType" = float32) -> WhisperEncoder:
    return WhisperEncoder(config, weights, dtype)


__all__ = ["WhisperEncoder", "WhisperEncoderLayer", "create_encoder"]
