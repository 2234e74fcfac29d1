"""Whisper decoder (reference: src/pygpukit/asr/whisper/decoder.py): token + learned position embedding, pre-norm layers of
causal self-attention, cross-attention over the encoder states and a GELU FFN, final layer norm, projection to the vocabulary.

Two ways through the same weights:

  * teacher-forced forward, `decoder(input_ids [B, S], encoder_hidden_states [B, S_enc, d]) -> logits [B, S, vocab]`: the
    reference's computation from the existing ops with no transposes - one q | k | v GEMM, sdpa_causal_strided reading that
    projection in place, the cross q GEMM, one k | v GEMM over the encoder rows, sdpa_noncausal_strided, linear_bias_gelu for
    fc1, the final norm and the bias-free output projection.  The reference materialises [H, S, S] scores between two batched
    matmuls and transposes eight times per layer;
  * the cached one-token step, `decode_step(token_id, position) -> logits [1, vocab]`: set_encoder_states() projects the encoder
    rows to K / V ONCE per layer into [H, S_enc, head_dim] cross caches (the reference re-projects all of them in every layer at
    every step and re-runs the whole prefix), self-attention K / V rows live in fixed caches, and the step is

        embed_token_position                                   token row + position row
        per layer  ln_linear_qkv_cache                         LN + q | k | v + bias, k / v written to the cache row
                   sdpa_fixed_cache (context from the device)  2 launches
                   ln_linear                                   out_proj + bias + residual
                   ln_linear                                   LN + cross q_proj + bias
                   sdpa_fixed_cache over the cross cache       2 launches
                   ln_linear                                   out_proj + bias + residual
                   ln_linear                                   LN + fc1 + bias + GELU
                   ln_linear                                   fc2 + bias + residual
        ln_linear                                              final LN + output projection
        argmax                                                 into a device slot

    10 launches per layer + 3 (decode_launches()).  Token id, position and context length live in one device int32 array, so
    the step's only host-to-device copy is that 12-byte upload, and capture_decode() / decode_step_graph() replay the step as
    one graph.  `fused=False` (or PGK_WHISPER_FUSED=0) runs the same cached step on the ops that predate ln_linear - layernorm,
    matmul_nt, gelu, add, kv_cache_update_gqa_ptr: 19 launches per layer + 6 - as a second opinion and a baseline.

The cached path serves one sequence (batch 1) and needs head_dim 64 or 128 (every Whisper size has 64)."""

from __future__ import annotations

import os
import re

import numpy as np

from pygpukit_amd.asr.whisper.config import WhisperConfig
from pygpukit_amd.asr.whisper.loader import WhisperWeights
from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import DataType, as_dtype, float32, int32
from pygpukit_amd.core.factory import from_numpy
from pygpukit_amd.core.stream import CudaGraph
from pygpukit_amd.ops._common import call
from pygpukit_amd.ops.elementwise import add
from pygpukit_amd.ops.embedding import embedding_lookup_batch, embedding_lookup_ptr, kv_cache_prefill_gqa, kv_cache_update_gqa_ptr
from pygpukit_amd.ops.matmul import linear_bias_gelu, matmul_nt
from pygpukit_amd.ops.nn.activation import gelu
from pygpukit_amd.ops.nn.attention import (_workspace, sdpa_causal_fixed_cache, sdpa_causal_fixed_cache_ptr, sdpa_causal_strided,
                                          sdpa_noncausal_strided)
from pygpukit_amd.ops.nn.linear import embed_token_position_ptr, ln_linear, ln_linear_qkv_cache_ptr, slice_rows_range_ptr
from pygpukit_amd.ops.nn.norm import layernorm
from pygpukit_amd.ops.reduction import argmax_int
from pygpukit_amd.ops.sampling import sample_token_gpu


def _flash_decoding_off() -> bool:
    """pgk_sdpa_fixed_cache's own switch (csrc/ops_attention.hip): set, not "auto", and an integer value of 0."""
    e = os.environ.get("PYGPUKIT_FLASH_DECODING")
    if e is None or e == "auto":
        return False
    m = re.match(r"\s*[+-]?\d+", e)
    return int(m.group()) == 0 if m else True                   # atoi: no leading digits reads as 0


def _to_gpu(arr, dtype: DataType) -> GPUArray:
    return from_numpy(np.ascontiguousarray(arr, dtype=np.float32)).astype(dtype)


def _bias_or_zeros(b, n: int) -> np.ndarray:
    return np.asarray(b, np.float32) if b is not None else np.zeros(n, np.float32)


class _StepBuffers:
    """Persistent buffers of the one-token step.  state = (token id, position, position + 1): one int32 array, one upload."""

    def __init__(self, config: WhisperConfig, dtype: DataType):
        d, H = config.d_model, config.decoder_attention_heads
        self.state = GPUArray((3,), int32)
        self.state.fill_zeros()
        self.token_buf, self.position_buf, self.context_buf = (self.state._view(i, (1,)) for i in range(3))
        self.hidden, self.q, self.attn, self.normed, self.proj = (GPUArray((1, d), dtype) for _ in range(5))
        self.q_heads, self.attn_heads = self.q.view((H, 1, d // H)), self.attn.view((H, 1, d // H))
        self.qkv = GPUArray((1, 3 * d), dtype)                   # unfused step only
        self.pos_row = GPUArray((1, d), dtype)
        self.ffn = GPUArray((1, config.decoder_ffn_dim), dtype)
        self.logits = GPUArray((1, config.vocab_size), dtype)
        self.next_token = GPUArray((1,), int32)
        self.next_token.fill_zeros()


class WhisperDecoderLayer:
    """x += self_attention(layer_norm(x)); x += cross_attention(layer_norm(x), encoder states); x += ffn(layer_norm(x))."""

    def __init__(self, config: WhisperConfig, layer_weights: dict, dtype: "str | DataType" = float32):
        self.config = config
        self.dtype = as_dtype(dtype)
        self.d_model = d = config.d_model
        self.n_heads = config.decoder_attention_heads
        self.head_dim = d // self.n_heads
        w = layer_weights
        cat = np.concatenate
        # q | k | v of self-attention and k | v of cross-attention as single weights; k_proj has no bias: zeros
        self.qkv_weight = _to_gpu(cat([w["self_attn_q_weight"], w["self_attn_k_weight"], w["self_attn_v_weight"]], axis=0), self.dtype)
        self.qkv_bias = _to_gpu(cat([w["self_attn_q_bias"], _bias_or_zeros(w.get("self_attn_k_bias"), d), w["self_attn_v_bias"]]), self.dtype)
        self.cross_kv_weight = _to_gpu(cat([w["cross_attn_k_weight"], w["cross_attn_v_weight"]], axis=0), self.dtype)
        self.cross_kv_bias = _to_gpu(cat([_bias_or_zeros(w.get("cross_attn_k_bias"), d), w["cross_attn_v_bias"]]), self.dtype)
        for name, key in (("out_weight", "self_attn_out_weight"), ("out_bias", "self_attn_out_bias"),
                          ("attn_ln_weight", "self_attn_layer_norm_weight"), ("attn_ln_bias", "self_attn_layer_norm_bias"),
                          ("cross_q_weight", "cross_attn_q_weight"), ("cross_q_bias", "cross_attn_q_bias"),
                          ("cross_out_weight", "cross_attn_out_weight"), ("cross_out_bias", "cross_attn_out_bias"),
                          ("cross_ln_weight", "cross_attn_layer_norm_weight"), ("cross_ln_bias", "cross_attn_layer_norm_bias"),
                          ("fc1_weight", "fc1_weight"), ("fc1_bias", "fc1_bias"), ("fc2_weight", "fc2_weight"), ("fc2_bias", "fc2_bias"),
                          ("ffn_ln_weight", "final_layer_norm_weight"), ("ffn_ln_bias", "final_layer_norm_bias")):
            setattr(self, name, _to_gpu(w[key], self.dtype))
        self.self_k: GPUArray | None = None          # [H, max_len, head_dim], init_cache
        self.self_v: GPUArray | None = None
        self.cross_k: GPUArray | None = None         # [H, S_enc, head_dim], set_encoder_states
        self.cross_v: GPUArray | None = None

    # ---- teacher-forced ---------------------------------------------------------------------------------------------
    def _project_encoder(self, enc: GPUArray) -> GPUArray:
        return matmul_nt(enc, self.cross_kv_weight, self.cross_kv_bias)                       # [S_enc, 2 d]: k | v per row

    def __call__(self, x: GPUArray, encoder_hidden_states: GPUArray) -> GPUArray:
        """x [S, d_model], encoder_hidden_states [S_enc, d_model] -> [S, d_model] (one batch element)."""
        d, hd, H = self.d_model, self.head_dim, self.n_heads
        if x.ndim != 2 or x.shape[1] != d or encoder_hidden_states.ndim != 2 or encoder_hidden_states.shape[1] != d:
            raise ValueError(f"WhisperDecoderLayer: x / encoder_hidden_states must be [rows, {d}], got {x.shape} / {encoder_hidden_states.shape}")
        S, S_enc = x.shape[0], encoder_hidden_states.shape[0]
        qkv = matmul_nt(layernorm(x, self.attn_ln_weight, self.attn_ln_bias), self.qkv_weight, self.qkv_bias)     # [S, 3 d]
        rest = qkv.size - 2 * d
        attn = GPUArray((S, d), x.dtype)
        sdpa_causal_strided(qkv, qkv._view(d, (rest,)), qkv._view(2 * d, (rest,)), attn, H, H, S, S, hd, (hd, 3 * d), (hd, 3 * d), (hd, d))
        x = add(x, matmul_nt(attn, self.out_weight, self.out_bias))
        q = matmul_nt(layernorm(x, self.cross_ln_weight, self.cross_ln_bias), self.cross_q_weight, self.cross_q_bias)
        kv = self._project_encoder(encoder_hidden_states)
        sdpa_noncausal_strided(q, kv, kv._view(d, (kv.size - d,)), attn, H, H, S, S_enc, hd, (hd, d), (hd, 2 * d), (hd, d))
        x = add(x, matmul_nt(attn, self.cross_out_weight, self.cross_out_bias))
        h = linear_bias_gelu(layernorm(x, self.ffn_ln_weight, self.ffn_ln_bias), self.fc1_weight, self.fc1_bias)
        return add(x, matmul_nt(h, self.fc2_weight, self.fc2_bias))

    # ---- caches -----------------------------------------------------------------------------------------------------
    def init_cache(self, max_len: int) -> None:
        shape = (self.n_heads, max_len, self.head_dim)
        self.self_k, self.self_v = GPUArray(shape, self.dtype), GPUArray(shape, self.dtype)
        self.self_k.fill_zeros()
        self.self_v.fill_zeros()

    def set_encoder_states(self, enc: GPUArray) -> None:
        """enc [S_enc, d]: ONE GEMM on the k | v weight and ONE cache write.  A row of the projection is 2 H heads (k heads, then
        v heads), so written as a [2 H, S_enc, head_dim] cache its first half is the K cache and its second the V cache."""
        S_enc, H, hd = enc.shape[0], self.n_heads, self.head_dim
        if self.cross_k is None or self.cross_k.shape[1] != S_enc:
            self._cross_kv = GPUArray((2 * H, S_enc, hd), self.dtype)
            self.cross_k, self.cross_v = self._cross_kv._view(0, (H, S_enc, hd)), self._cross_kv._view(H * S_enc * hd, (H, S_enc, hd))
        kv_cache_prefill_gqa(self._project_encoder(enc).view((S_enc, 2 * H, hd)), self._cross_kv, 2 * H, 0)

    # ---- one token ------------------------------------------------------------------------------------------------------
    def decode_fused(self, b: _StepBuffers) -> None:
        """b.hidden updated in place: 10 launches, persistent buffers only."""
        ln_linear_qkv_cache_ptr(b.hidden, self.qkv_weight, self.qkv_bias, b.q, self.self_k, self.self_v, b.position_buf,
                                gamma=self.attn_ln_weight, beta=self.attn_ln_bias)
        sdpa_causal_fixed_cache_ptr(b.q_heads, self.self_k, self.self_v, b.attn_heads, b.context_buf, self.self_k.shape[1])
        ln_linear(b.attn, self.out_weight, self.out_bias, residual=b.hidden, out=b.hidden)
        ln_linear(b.hidden, self.cross_q_weight, self.cross_q_bias, gamma=self.cross_ln_weight, beta=self.cross_ln_bias, out=b.q)
        sdpa_causal_fixed_cache(b.q_heads, self.cross_k, self.cross_v, b.attn_heads, self.cross_k.shape[1])
        ln_linear(b.attn, self.cross_out_weight, self.cross_out_bias, residual=b.hidden, out=b.hidden)
        ln_linear(b.hidden, self.fc1_weight, self.fc1_bias, gamma=self.ffn_ln_weight, beta=self.ffn_ln_bias, activation="gelu", out=b.ffn)
        ln_linear(b.ffn, self.fc2_weight, self.fc2_bias, residual=b.hidden, out=b.hidden)

    def decode_unfused(self, b: _StepBuffers) -> None:
        """The same step on layernorm, matmul_nt, gelu, add and the cache-write op: 19 launches."""
        d, H, hd = self.d_model, self.n_heads, self.head_dim
        layernorm(b.hidden, self.attn_ln_weight, self.attn_ln_bias, out=b.normed)
        matmul_nt(b.normed, self.qkv_weight, self.qkv_bias, out=b.qkv)
        kv_cache_update_gqa_ptr(b.qkv._view(d, (1, H, hd)), self.self_k, H, b.position_buf)
        kv_cache_update_gqa_ptr(b.qkv._view(2 * d, (1, H, hd)), self.self_v, H, b.position_buf)
        sdpa_causal_fixed_cache_ptr(b.qkv._view(0, (H, 1, hd)), self.self_k, self.self_v, b.attn_heads, b.context_buf, self.self_k.shape[1])
        matmul_nt(b.attn, self.out_weight, self.out_bias, out=b.proj)
        add(b.hidden, b.proj, out=b.hidden)
        layernorm(b.hidden, self.cross_ln_weight, self.cross_ln_bias, out=b.normed)
        matmul_nt(b.normed, self.cross_q_weight, self.cross_q_bias, out=b.q)
        sdpa_causal_fixed_cache(b.q_heads, self.cross_k, self.cross_v, b.attn_heads, self.cross_k.shape[1])
        matmul_nt(b.attn, self.cross_out_weight, self.cross_out_bias, out=b.proj)
        add(b.hidden, b.proj, out=b.hidden)
        layernorm(b.hidden, self.ffn_ln_weight, self.ffn_ln_bias, out=b.normed)
        matmul_nt(b.normed, self.fc1_weight, self.fc1_bias, out=b.ffn)
        gelu(b.ffn, out=b.ffn)
        matmul_nt(b.ffn, self.fc2_weight, self.fc2_bias, out=b.proj)
        add(b.hidden, b.proj, out=b.hidden)


class WhisperDecoder:
    def __init__(self, config: WhisperConfig, weights: WhisperWeights, dtype: "str | DataType" = float32, *, fused: bool | None = None):
        if weights.decoder_embed_tokens is None or not weights.decoder_layers:
            raise ValueError("WhisperDecoder: the weights hold no decoder tensors (model.decoder.* missing from the loaded dict)")
        if config.d_model % config.decoder_attention_heads:
            raise ValueError(f"WhisperDecoder: d_model {config.d_model} is no multiple of {config.decoder_attention_heads} heads")
        self.config = config
        self.dtype = as_dtype(dtype)
        self.d_model = config.d_model
        self.n_layers = config.decoder_layers
        self.vocab_size = config.vocab_size
        self.n_heads = config.decoder_attention_heads
        self.head_dim = config.d_model // config.decoder_attention_heads
        self.fused = (os.environ.get("PGK_WHISPER_FUSED", "1") != "0") if fused is None else bool(fused)
        self.embed_tokens = _to_gpu(weights.decoder_embed_tokens, self.dtype)
        self.embed_positions = _to_gpu(weights.decoder_embed_positions, self.dtype)
        self.layer_norm_weight = _to_gpu(weights.decoder_layer_norm_weight, self.dtype)
        self.layer_norm_bias = _to_gpu(weights.decoder_layer_norm_bias, self.dtype)
        self.proj_out = _to_gpu(weights.proj_out_weight, self.dtype)
        if self.proj_out.shape != (self.vocab_size, self.d_model) or self.embed_tokens.shape != (self.vocab_size, self.d_model):
            raise ValueError(f"WhisperDecoder: embed_tokens {self.embed_tokens.shape} / proj_out {self.proj_out.shape} are not [{self.vocab_size}, {self.d_model}]")
        self.max_positions = min(config.max_target_positions, self.embed_positions.shape[0])
        self.layers = [WhisperDecoderLayer(config, lw, self.dtype) for lw in weights.decoder_layers]
        self.max_cache_len = 0                       # rows of the self-attention caches; 0: init_cache not called
        self.encoder_rows = 0                        # rows of the cross caches; 0: set_encoder_states not called
        self._step: _StepBuffers | None = None
        self._graph: CudaGraph | None = None

    # ---- teacher-forced forward -------------------------------------------------------------------------------------------
    def __call__(self, input_ids, encoder_hidden_states: GPUArray, past_key_values=None) -> GPUArray:
        """input_ids [B, S] (ndarray or GPUArray of integers), encoder_hidden_states [B, S_enc, d_model] -> logits [B, S, vocab]."""
        if past_key_values is not None:
            raise ValueError("WhisperDecoder: past_key_values is not supported - the cached path is set_encoder_states / decode_step")
        ids = np.asarray(input_ids.to_numpy() if isinstance(input_ids, GPUArray) else input_ids).astype(np.int64)
        enc = encoder_hidden_states
        if ids.ndim != 2 or ids.shape[1] < 1:
            raise ValueError(f"WhisperDecoder: input_ids must be [batch, seq_len >= 1], got {ids.shape}")
        if enc.ndim != 3 or enc.shape[0] != ids.shape[0] or enc.shape[2] != self.d_model or enc.shape[1] < 1:
            raise ValueError(f"WhisperDecoder: encoder_hidden_states must be [{ids.shape[0]}, rows, {self.d_model}], got {enc.shape}")
        B, S = ids.shape
        if S > self.max_positions:
            raise ValueError(f"WhisperDecoder: {S} tokens exceed max_target_positions {self.max_positions}")
        if ids.min() < 0 or ids.max() >= self.vocab_size:
            raise ValueError(f"WhisperDecoder: token id outside [0, {self.vocab_size})")
        enc = enc.astype(self.dtype)
        S_enc, d, V = enc.shape[1], self.d_model, self.vocab_size
        logits = GPUArray((B, S, V), self.dtype)
        positions = self.embed_positions._view(0, (S, d))
        for b in range(B):
            x = GPUArray((S, d), self.dtype)
            embedding_lookup_batch(self.embed_tokens, x, from_numpy(ids[b].astype(np.int32)), S)
            x = add(x, positions)
            e = enc._view(b * S_enc * d, (S_enc, d))
            for layer in self.layers:
                x = layer(x, e)
            x = layernorm(x, self.layer_norm_weight, self.layer_norm_bias)
            matmul_nt(x, self.proj_out, out=logits._view(b * S * V, (S, V)))
        return logits

    # ---- caches -----------------------------------------------------------------------------------------------------------
    def init_cache(self, max_len: int | None = None) -> None:
        """Allocate (zeroed) self-attention caches [H, max_len, head_dim] per layer (default max_target_positions) and the step
        buffers.  A captured graph addresses the old caches, so it is dropped: capture_decode() again."""
        max_len = self.max_positions if max_len is None else int(max_len)
        if not 1 <= max_len <= self.max_positions:
            raise ValueError(f"WhisperDecoder.init_cache: max_len {max_len} outside [1, {self.max_positions}]")
        if self.head_dim not in (64, 128):
            raise ValueError(f"WhisperDecoder.init_cache: the cached step needs head_dim 64 or 128, got {self.head_dim}")
        for layer in self.layers:
            layer.init_cache(max_len)
        self._step = _StepBuffers(self.config, self.dtype)
        _workspace(self.n_heads, self.head_dim, max_len)             # the attention op must not allocate under capture
        self.max_cache_len = max_len
        self._graph = None

    def set_encoder_states(self, encoder_hidden_states: GPUArray) -> None:
        """encoder_hidden_states [1, S_enc, d_model] (or [S_enc, d_model]): project K / V of every layer's cross-attention
        once.  Runs once per audio.  The self-attention caches need no clearing: a step reads rows below its own position only
        and generation starts again at position 0.  A different S_enc replaces the cross caches and drops a captured graph."""
        enc = encoder_hidden_states
        if enc.ndim == 3:
            if enc.shape[0] != 1:
                raise ValueError(f"WhisperDecoder.set_encoder_states: the cached path serves one sequence, got batch {enc.shape[0]}")
            enc = enc._view(0, enc.shape[1:])
        if enc.ndim != 2 or enc.shape[1] != self.d_model or enc.shape[0] < 1:
            raise ValueError(f"WhisperDecoder.set_encoder_states: expected [1, rows, {self.d_model}], got {encoder_hidden_states.shape}")
        if self.max_cache_len == 0:
            self.init_cache()
        enc = enc.astype(self.dtype)
        if enc.shape[0] != self.encoder_rows:
            self._graph = None
        for layer in self.layers:
            layer.set_encoder_states(enc)
        self.encoder_rows = enc.shape[0]
        _workspace(self.n_heads, self.head_dim, self.encoder_rows)

    # ---- one-token step ---------------------------------------------------------------------------------------------------
    def decode_launches(self) -> int:
        """Kernel launches of one cached step.  fused: per layer 6 ln_linear (one with the cache write) + 2 attention ops of 2
        launches each = 10, plus embed_token_position, the final ln_linear and argmax.  Unfused: per layer 3 layernorm, 6
        matmul_nt, 2 cache writes, gelu, 3 add and 2 attention ops of 2 = 19, plus embedding, position row, add, final
        layernorm, projection and argmax.  The attention op takes its two-kernel path with the workspace allocated by
        init_cache / set_encoder_states and its 16-byte-aligned persistent buffers; the cross call passes its context length from
        the host, so PYGPUKIT_FLASH_DECODING=0 (read per call by the library) sends it to the one-launch general kernel, which
        works in LDS alone: one launch fewer per layer, still nothing allocated."""
        self_attn = 2                                # sdpa_fixed_cache, context on the device: always split pass + merge pass
        cross_attn = 1 if _flash_decoding_off() else 2
        if self.fused:
            return self.n_layers * (6 + self_attn + cross_attn) + 3
        return self.n_layers * (3 + 6 + 2 + 1 + 3 + self_attn + cross_attn) + 6

    def _set_state(self, token_id: int, position: int, name: str) -> _StepBuffers:
        if self._step is None or self.encoder_rows == 0:
            raise RuntimeError(f"WhisperDecoder.{name}: call set_encoder_states() first")
        if not 0 <= token_id < self.vocab_size:
            raise ValueError(f"WhisperDecoder.{name}: token id {token_id} outside [0, {self.vocab_size})")
        if not 0 <= position < self.max_cache_len:
            raise ValueError(f"WhisperDecoder.{name}: position {position} outside the cache of {self.max_cache_len} rows")
        self._step.state.copy_from_numpy(np.array([token_id, position, position + 1], np.int32))      # the step's only upload
        return self._step

    def _decode_ops(self, b: _StepBuffers) -> None:
        """The one-token step on the persistent buffers: no allocation, no host value - safe to capture."""
        if self.fused:
            embed_token_position_ptr(self.embed_tokens, self.embed_positions, b.hidden, b.state)
            for layer in self.layers:
                layer.decode_fused(b)
            ln_linear(b.hidden, self.proj_out, None, gamma=self.layer_norm_weight, beta=self.layer_norm_bias, out=b.logits)
        else:
            embedding_lookup_ptr(self.embed_tokens, b.hidden, b.token_buf)
            slice_rows_range_ptr(self.embed_positions, b.pos_row, b.position_buf, 1)
            add(b.hidden, b.pos_row, out=b.hidden)
            for layer in self.layers:
                layer.decode_unfused(b)
            layernorm(b.hidden, self.layer_norm_weight, self.layer_norm_bias, out=b.normed)
            matmul_nt(b.normed, self.proj_out, out=b.logits)
        call("pgk_argmax", b.logits._p, 1, self.vocab_size, self.dtype.code, b.next_token._p, None)

    def decode_step(self, token_id: int, position: int) -> GPUArray:
        """token_id at `position` against self-cache rows 0 .. position-1 (its own row is written first) and the cross caches
        -> logits [1, vocab]: the decoder's persistent buffer, valid until the next step.  The argmax is left in a device slot
        (next_token())."""
        b = self._set_state(int(token_id), int(position), "decode_step")
        self._decode_ops(b)
        return b.logits

    def next_token(self) -> int:
        """The argmax of the last step's logits (one 4-byte copy)."""
        if self._step is None:
            raise RuntimeError("WhisperDecoder.next_token: no step has run")
        return int(self._step.next_token.to_numpy()[0])

    def capture_decode(self) -> None:
        """Capture the whole one-token step as one graph on one stream."""
        if self._step is None or self.encoder_rows == 0:
            raise RuntimeError("WhisperDecoder.capture_decode: call set_encoder_states() first")
        graph = CudaGraph()
        graph.begin_capture()
        try:
            self._decode_ops(self._step)
        finally:
            graph.end_capture()
        self._graph = graph

    def decode_step_graph(self, token_id: int, position: int) -> GPUArray:
        """decode_step as the state upload + one graph replay; same logits buffer."""
        if self._graph is None:
            raise RuntimeError("WhisperDecoder.decode_step_graph: nothing captured for the current caches - call capture_decode() "
                               "(again after init_cache or encoder states of another length)")
        b = self._set_state(int(token_id), int(position), "decode_step_graph")
        self._graph.replay()
        return b.logits

    # ---- generation ---------------------------------------------------------------------------------------------------------
    def generate(self, encoder_hidden_states: GPUArray, max_length: int = 448, temperature: float = 1.0, top_k: int | None = None, *,
                 prompt_ids=None, use_cache: bool = True, use_graph: bool = False, seed: int | None = None) -> list[int]:
        """The reference's loop: start from decoder_start_token_id (or prompt_ids, fed one token per step), greedy when top_k is
        None whatever the temperature, stop after eos_token_id.  max_length counts every token returned and is clamped to
        max_target_positions (the reference would index past its position table).  With top_k the token comes from
        sample_token_gpu with u drawn from np.random.default_rng(seed): deterministic for a seed, not the reference's
        np.random.choice stream.  use_cache=False is the reference's loop over the teacher-forced forward."""
        if use_graph and not use_cache:
            raise ValueError("WhisperDecoder.generate: use_graph=True needs use_cache=True")
        if top_k is not None and top_k < 1:
            raise ValueError(f"WhisperDecoder.generate: top_k must be >= 1, got {top_k}")
        tokens = [int(t) for t in prompt_ids] if prompt_ids is not None else [int(self.config.decoder_start_token_id)]
        if not tokens:
            raise ValueError("WhisperDecoder.generate: empty prompt_ids")
        limit = self.max_positions
        if use_cache:
            self.set_encoder_states(encoder_hidden_states)
            limit = min(limit, self.max_cache_len)
            if use_graph and self._graph is None:
                self.capture_decode()
        max_length = min(int(max_length), limit)
        if len(tokens) >= max_length:
            return tokens[:max_length] if len(tokens) > max_length else tokens
        rng = np.random.default_rng(seed)
        t_sample = float(temperature) if temperature > 0.0 else 1.0
        step = self.decode_step_graph if use_graph else self.decode_step

        def pick(row: GPUArray, greedy_slot: bool) -> int:
            if top_k is not None:
                return sample_token_gpu(row, t_sample, int(top_k), 1.0, u=float(rng.random(dtype=np.float32)))
            return self.next_token() if greedy_slot else argmax_int(row)

        if use_cache:
            logits = None
            for pos, t in enumerate(tokens):
                logits = step(t, pos)
        while len(tokens) < max_length:
            if use_cache:
                nxt = pick(logits, True)
            else:
                full = self(np.array([tokens], dtype=np.int64), encoder_hidden_states)
                nxt = pick(full._view((len(tokens) - 1) * self.vocab_size, (self.vocab_size,)), False)
            tokens.append(nxt)
            if nxt == self.config.eos_token_id or len(tokens) >= max_length:
                break
            if use_cache:
                logits = step(nxt, len(tokens) - 1)
        return tokens


def create_decoder(config: WhisperConfig, weights: WhisperWeights, dtype: "str | DataType" = float32, **kwargs) -> WhisperDecoder:
    return WhisperDecoder(config, weights, dtype, **kwargs)


__all__ = ["WhisperDecoder", "WhisperDecoderLayer", "create_decoder"]
