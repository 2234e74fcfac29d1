"""Llama 4 text model (reference: src/pygpukit/llm/models/llama4.py:29-407; HuggingFace Llama4ForCausalLM).

Per block: RMSNorm -> q/k/v projections -> parameterless L2 norm on Q and K (use_qk_norm; as in the reference on every
layer, whatever use_rope says) -> sdpa_irope (positions 0..S-1, offset 0) -> o_proj + residual -> RMSNorm ->
down(silu(gate) * up) + residual; then the final norm and lm_head.  Same classes, signatures and arithmetic as the
reference; the data movement is this project's:
  * weights stay [out, in] as stored (matmul_nt), no transposed copies;
  * attention reads Q, K, V in their [S, H*D] projection layout through sdpa_irope_strided and writes [S, Hq*D]: no
    [S,H,D] <-> [H,S,D] transposes, and the L2 norm runs in place on the projection buffers;
  * the embedding rows are gathered on the device.
`generate` re-runs `forward` on the growing sequence, like the reference (no KV cache for this model yet)."""

from __future__ import annotations

import json
import os
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import bfloat16, float16, float32
from pygpukit_amd.core.factory import from_numpy
from pygpukit_amd.ops.basic import add, embedding_lookup_batch, matmul_nt, rmsnorm, swiglu
from pygpukit_amd.ops.nn import l2norm, sdpa_irope_strided


@dataclass
class Llama4Config:
    """Llama 4 text model configuration."""

    vocab_size: int = 202048
    hidden_size: int = 5120
    intermediate_size: int = 8192
    num_hidden_layers: int = 48
    num_attention_heads: int = 40
    num_key_value_heads: int = 8
    head_dim: int = 128
    rms_norm_eps: float = 1e-5
    attn_scale: float = 0.1
    floor_scale: float = 8192.0
    use_qk_norm: bool = True
    max_position_embeddings: int = 10485760
    no_rope_layers: list[int] | None = None  # 1 = NoPE (no RoPE), 0 = RoPE

    @classmethod
    def from_json(cls, path: str | Path) -> "Llama4Config":
        """Load from a HuggingFace config.json (the text model may be nested under "text_config")."""
        with open(path, encoding="utf-8") as f:
            data = json.load(f)
        text_config = data.get("text_config", data)
        default = cls()
        return cls(**{name: text_config.get(name, getattr(default, name)) for name in cls.__dataclass_fields__})


class Llama4Attention:
    """Attention with QK L2 norm and iRoPE temperature scaling; projections are [out, in]."""

    def __init__(self, q_proj: GPUArray, k_proj: GPUArray, v_proj: GPUArray, o_proj: GPUArray, config: Llama4Config,
                 use_rope: bool = True):
        self.q_proj, self.k_proj, self.v_proj, self.o_proj = q_proj, k_proj, v_proj, o_proj
        self.config = config
        self.use_rope = use_rope
        self.num_heads = config.num_attention_heads
        self.num_kv_heads = config.num_key_value_heads
        self.head_dim = config.head_dim

    def forward(self, hidden: GPUArray, positions: GPUArray) -> GPUArray:
        """hidden [seq_len, hidden_size], positions [seq_len] int64 / int32 -> [seq_len, hidden_size]."""
        S, Hq, Hkv, D = hidden.shape[0], self.num_heads, self.num_kv_heads, self.head_dim
        q = matmul_nt(hidden, self.q_proj)      # [S, Hq * D]
        k = matmul_nt(hidden, self.k_proj)      # [S, Hkv * D]
        v = matmul_nt(hidden, self.v_proj)
        if self.config.use_qk_norm:
            qf, kf = q.view((S * Hq, D)), k.view((S * Hkv, D))
            l2norm(qf, eps=self.config.rms_norm_eps, out=qf)
            l2norm(kf, eps=self.config.rms_norm_eps, out=kf)
        attn = GPUArray((S, Hq * D), hidden.dtype)
        sdpa_irope_strided(q, k, v, positions, attn, Hq, Hkv, S, S, D, (D, Hq * D), (D, Hkv * D), (D, Hq * D),
                           attn_scale=self.config.attn_scale, floor_scale=self.config.floor_scale, causal_offset=0)
        return matmul_nt(attn, self.o_proj)


class Llama4MLP:
    """down_proj(silu(gate_proj(x)) * up_proj(x)); projections are [out, in]."""

    def __init__(self, gate_proj: GPUArray, up_proj: GPUArray, down_proj: GPUArray):
        self.gate_proj, self.up_proj, self.down_proj = gate_proj, up_proj, down_proj

    def forward(self, hidden: GPUArray) -> GPUArray:
        gate = matmul_nt(hidden, self.gate_proj)
        up = matmul_nt(hidden, self.up_proj)
        return matmul_nt(swiglu(gate, up, out=gate), self.down_proj)


class Llama4Block:
    """Single Llama 4 transformer block."""

    def __init__(self, attn: Llama4Attention, mlp: Llama4MLP, input_norm_weight: GPUArray, post_attn_norm_weight: GPUArray,
                 rms_norm_eps: float):
        self.attn, self.mlp = attn, mlp
        self.input_norm_weight, self.post_attn_norm_weight = input_norm_weight, post_attn_norm_weight
        self.rms_norm_eps = rms_norm_eps

    def forward(self, hidden: GPUArray, positions: GPUArray) -> GPUArray:
        normed = rmsnorm(hidden, self.input_norm_weight, self.rms_norm_eps)
        hidden = add(hidden, self.attn.forward(normed, positions))
        normed = rmsnorm(hidden, self.post_attn_norm_weight, self.rms_norm_eps)
        return add(hidden, self.mlp.forward(normed))


class Llama4Model:
    """Llama 4 text model for inference."""

    def __init__(self, config: Llama4Config, embed_tokens: GPUArray, blocks: list[Llama4Block], final_norm_weight: GPUArray,
                 lm_head: GPUArray):
        self.config = config
        self.embed_tokens = embed_tokens
        self.blocks = blocks
        self.final_norm_weight = final_norm_weight
        self.lm_head = lm_head

    def forward(self, input_ids: np.ndarray) -> GPUArray:
        """input_ids [seq_len] -> logits [seq_len, vocab_size]."""
        ids = np.asarray(input_ids).astype(np.int64).ravel()
        S = int(ids.shape[0])
        if S < 1:
            raise ValueError("Llama4Model.forward: empty input_ids")
        if ids.min() < 0 or ids.max() >= self.embed_tokens.shape[0]:
            raise ValueError(f"Llama4Model.forward: token id outside [0, {self.embed_tokens.shape[0]})")
        hidden = GPUArray((S, self.embed_tokens.shape[1]), self.embed_tokens.dtype)
        embedding_lookup_batch(self.embed_tokens, hidden, from_numpy(ids.astype(np.int32)), S)
        positions = from_numpy(np.arange(S, dtype=np.int64))
        for block in self.blocks:
            hidden = block.forward(hidden, positions)
        hidden = rmsnorm(hidden, self.final_norm_weight, self.config.rms_norm_eps)
        return matmul_nt(hidden, self.lm_head)

    @classmethod
    def from_safetensors(cls, model_path: str | Path) -> "Llama4Model":
        """Load from a directory holding config.json and model.safetensors.index.json (+ shards) or model.safetensors;
        tensor names are language_model.model.* / language_model.lm_head.weight."""
        from pygpukit_amd.llm.safetensors import Dtype, load_safetensors

        model_path = Path(model_path)
        config = Llama4Config.from_json(model_path / "config.json")
        index = model_path / "model.safetensors.index.json"
        st = load_safetensors(str(index if os.path.exists(index) else model_path / "model.safetensors"))
        dtypes = {Dtype.BFloat16: bfloat16, Dtype.Float16: float16, Dtype.Float32: float32}

        def get_weight(name: str) -> GPUArray:
            info = st.tensor_info(name)
            if info.dtype not in dtypes:
                raise ValueError(f"Unsupported dtype: {info.dtype_name}")
            w = GPUArray(tuple(info.shape), dtypes[info.dtype])
            st.upload(name, w)          # file mapping -> device, [out, in] as stored
            return w

        embed_tokens = get_weight("language_model.model.embed_tokens.weight")
        blocks = []
        for i in range(config.num_hidden_layers):
            prefix = f"language_model.model.layers.{i}"
            use_rope = True
            if config.no_rope_layers is not None and i < len(config.no_rope_layers):
                use_rope = config.no_rope_layers[i] == 0
            attn = Llama4Attention(*(get_weight(f"{prefix}.self_attn.{p}_proj.weight") for p in "qkvo"), config, use_rope=use_rope)
            mlp = Llama4MLP(*(get_weight(f"{prefix}.feed_forward.{p}_proj.weight") for p in ("gate", "up", "down")))
            blocks.append(Llama4Block(attn, mlp, get_weight(f"{prefix}.input_layernorm.weight"),
                                      get_weight(f"{prefix}.post_attention_layernorm.weight"), config.rms_norm_eps))
        final_norm = get_weight("language_model.model.norm.weight")
        lm_head = get_weight("language_model.lm_head.weight")
        return cls(config, embed_tokens, blocks, final_norm, lm_head)


def generate(model: Llama4Model, input_ids: np.ndarray, max_new_tokens: int = 50, eos_token_id: int | list[int] = 200001) -> np.ndarray:
    """Greedy generation; returns the token ids including the input."""
    eos_token_ids = {eos_token_id} if isinstance(eos_token_id, int) else set(eos_token_id)
    current_ids = [int(t) for t in input_ids]
    for _ in range(max_new_tokens):
        logits = model.forward(np.array(current_ids, dtype=np.int64))
        last = logits.to_numpy()[-1]
        if last.dtype == np.uint16:     # bfloat16 words
            last = (last.astype(np.uint32) << 16).view(np.float32)
        next_token = int(np.argmax(last))
        current_ids.append(next_token)
        if next_token in eos_token_ids:
            break
    return np.array(current_ids, dtype=np.int64)
