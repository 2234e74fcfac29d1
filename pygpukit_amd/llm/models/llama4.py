"""Llama 4 text model (reference: src/pygpukit/llm/models/llama4.py:29-407; HuggingFace Llama4ForCausalLM).

Per block: RMSNorm -> q/k/v projections -> parameterless L2 norm on Q and K (use_qk_norm; as in the reference on every
layer, whatever use_rope says) -> sdpa_irope (positions 0..S-1, offset 0) -> o_proj + residual -> RMSNorm ->
down(silu(gate) * up) + residual; then the final norm and lm_head.  Same classes, signatures and arithmetic as the
reference; the data movement is this project's:
  * weights stay [out, in] as stored (matmul_nt), no transposed copies;
  * attention reads Q, K, V in their [S, H*D] projection layout through sdpa_irope_strided and writes [S, Hq*D]: no
    [S,H,D] <-> [H,S,D] transposes, and the L2 norm runs in place on the projection buffers;
  * the embedding rows are gathered on the device.
`generate` re-runs `forward` on the growing sequence, like the reference, unless use_cache=True.

KV-cache decode (build-defined; the reference has none for this model): `init_fixed_cache` allocates per-layer caches
[Hkv, max_seq, D] and the one-token buffers, `prefill_fixed_cache` runs `forward`'s op sequence with attention reading
the cache (so a prompt may come in chunks), `decode_step` runs one token through the _ptr ops on the persistent buffers
(token id and position live in device memory), and `capture_decode` / `decode_step_graph` replay that step as one graph.
Per layer a cached step is llama4_qk_norm_cache_write + sdpa_irope_fixed_cache between the projections."""

from __future__ import annotations

import json
import os
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import bfloat16, float16, float32, int32
from pygpukit_amd.core.factory import from_numpy
from pygpukit_amd.core.stream import CudaGraph
from pygpukit_amd.ops.basic import add, add_inplace, embedding_lookup_batch, embedding_lookup_ptr, matmul_nt, rmsnorm, swiglu
from pygpukit_amd.ops.nn import (l2norm, llama4_qk_norm_cache_write, llama4_qk_norm_cache_write_ptr, sdpa_irope_fixed_cache_ptr,
                                 sdpa_irope_strided)
from pygpukit_amd.ops.nn.attention import _workspace


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
        self._k_cache: GPUArray | None = None       # [Hkv, max_seq, D], init_fixed_cache
        self._v_cache: GPUArray | None = None

    def init_fixed_cache(self, max_seq_len: int, dtype) -> None:
        shape = (self.num_kv_heads, max_seq_len, self.head_dim)
        self._k_cache, self._v_cache = GPUArray(shape, dtype), GPUArray(shape, dtype)
        self._k_cache.fill_zeros()
        self._v_cache.fill_zeros()

    def _qk_norm_args(self) -> dict:
        return dict(num_heads=self.num_heads, num_kv_heads=self.num_kv_heads, head_dim=self.head_dim, eps=self.config.rms_norm_eps,
                    qk_norm=self.config.use_qk_norm)

    def prefill_fixed_cache(self, hidden: GPUArray, positions: GPUArray, start_pos: int) -> GPUArray:
        """`forward` for rows start_pos .. start_pos+S-1 with K / V going to the cache and attention reading it."""
        S, Hq, Hkv, D = hidden.shape[0], self.num_heads, self.num_kv_heads, self.head_dim
        q = matmul_nt(hidden, self.q_proj)
        k = matmul_nt(hidden, self.k_proj)
        v = matmul_nt(hidden, self.v_proj)
        llama4_qk_norm_cache_write(q, k, v, self._k_cache, self._v_cache, start_pos, **self._qk_norm_args())
        attn = GPUArray((S, Hq * D), hidden.dtype)
        max_seq = self._k_cache.shape[1]
        sdpa_irope_strided(q, self._k_cache, self._v_cache, positions, attn, Hq, Hkv, S, start_pos + S, D, (D, Hq * D), (max_seq * D, D),
                           (D, Hq * D), attn_scale=self.config.attn_scale, floor_scale=self.config.floor_scale, causal_offset=start_pos)
        return matmul_nt(attn, self.o_proj)

    def decode_fixed_cache(self, b: "_DecodeBuffers") -> None:
        """One token: b.normed -> b.proj, through the cache row at b.position_buf[0].  Writes only persistent buffers."""
        matmul_nt(b.normed, self.q_proj, out=b.q)
        matmul_nt(b.normed, self.k_proj, out=b.k)
        matmul_nt(b.normed, self.v_proj, out=b.v)
        llama4_qk_norm_cache_write_ptr(b.q, b.k, b.v, self._k_cache, self._v_cache, b.position_buf, **self._qk_norm_args())
        sdpa_irope_fixed_cache_ptr(b.q_heads, self._k_cache, self._v_cache, b.attn_heads, b.position_buf, self.config.attn_scale,
                                   self.config.floor_scale)
        matmul_nt(b.attn, self.o_proj, out=b.proj)

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

    def decode_fixed_cache(self, b: "_DecodeBuffers") -> None:
        """One token: b.normed -> b.proj."""
        matmul_nt(b.normed, self.gate_proj, out=b.gate)
        matmul_nt(b.normed, self.up_proj, out=b.up)
        swiglu(b.gate, b.up, out=b.gate)
        matmul_nt(b.gate, self.down_proj, out=b.proj)


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

    def prefill_fixed_cache(self, hidden: GPUArray, positions: GPUArray, start_pos: int) -> GPUArray:
        normed = rmsnorm(hidden, self.input_norm_weight, self.rms_norm_eps)
        hidden = add(hidden, self.attn.prefill_fixed_cache(normed, positions, start_pos))
        normed = rmsnorm(hidden, self.post_attn_norm_weight, self.rms_norm_eps)
        return add(hidden, self.mlp.forward(normed))

    def decode_fixed_cache(self, b: "_DecodeBuffers") -> None:
        """One token, b.hidden updated in place."""
        rmsnorm(b.hidden, self.input_norm_weight, self.rms_norm_eps, out=b.normed)
        self.attn.decode_fixed_cache(b)
        add_inplace(b.hidden, b.proj)
        rmsnorm(b.hidden, self.post_attn_norm_weight, self.rms_norm_eps, out=b.normed)
        self.mlp.decode_fixed_cache(b)
        add_inplace(b.hidden, b.proj)


class _DecodeBuffers:
    """The persistent buffers of the one-token step: token id and position (one int32[2] array, so the host updates both
    with a single 8-byte copy) and every activation."""

    def __init__(self, config: Llama4Config, dtype):
        H, Hq, Hkv, D = config.hidden_size, config.num_attention_heads, config.num_key_value_heads, config.head_dim
        self.state = GPUArray((2,), int32)
        self.state.fill_zeros()
        self.token_id_buf, self.position_buf = self.state._view(0, (1,)), self.state._view(1, (1,))
        self.hidden, self.normed, self.proj = (GPUArray((1, H), dtype) for _ in range(3))
        self.q, self.attn = GPUArray((1, Hq * D), dtype), GPUArray((1, Hq * D), dtype)
        self.k, self.v = GPUArray((1, Hkv * D), dtype), GPUArray((1, Hkv * D), dtype)
        self.q_heads, self.attn_heads = self.q.view((Hq, 1, D)), self.attn.view((Hq, 1, D))
        self.gate, self.up = GPUArray((1, config.intermediate_size), dtype), GPUArray((1, config.intermediate_size), dtype)
        self.logits = GPUArray((1, config.vocab_size), dtype)


class Llama4Model:
    """Llama 4 text model for inference."""

    def __init__(self, config: Llama4Config, embed_tokens: GPUArray, blocks: list[Llama4Block], final_norm_weight: GPUArray,
                 lm_head: GPUArray):
        self.config = config
        self.embed_tokens = embed_tokens
        self.blocks = blocks
        self.final_norm_weight = final_norm_weight
        self.lm_head = lm_head
        self.max_cache_len = 0                          # rows of the fixed caches; 0: init_fixed_cache not called
        self._decode: _DecodeBuffers | None = None
        self._graph: CudaGraph | None = None

    def _embed(self, input_ids, name: str) -> tuple[GPUArray, int]:
        ids = np.asarray(input_ids).astype(np.int64).ravel()
        S = int(ids.shape[0])
        if S < 1:
            raise ValueError(f"Llama4Model.{name}: empty input_ids")
        if ids.min() < 0 or ids.max() >= self.embed_tokens.shape[0]:
            raise ValueError(f"Llama4Model.{name}: token id outside [0, {self.embed_tokens.shape[0]})")
        hidden = GPUArray((S, self.embed_tokens.shape[1]), self.embed_tokens.dtype)
        embedding_lookup_batch(self.embed_tokens, hidden, from_numpy(ids.astype(np.int32)), S)
        return hidden, S

    def forward(self, input_ids: np.ndarray) -> GPUArray:
        """input_ids [seq_len] -> logits [seq_len, vocab_size]."""
        hidden, S = self._embed(input_ids, "forward")
        positions = from_numpy(np.arange(S, dtype=np.int64))
        for block in self.blocks:
            hidden = block.forward(hidden, positions)
        hidden = rmsnorm(hidden, self.final_norm_weight, self.config.rms_norm_eps)
        return matmul_nt(hidden, self.lm_head)

    # ---- KV-cache decode -----------------------------------------------------------------------------------------
    def init_fixed_cache(self, max_seq_len: int) -> None:
        """Allocate (zeroed) per-layer K / V caches [Hkv, max_seq_len, D] in the model dtype and the one-token buffers.
        A captured decode graph addresses the old caches, so it is dropped: capture_decode() again."""
        if max_seq_len < 1:
            raise ValueError(f"Llama4Model.init_fixed_cache: max_seq_len must be >= 1, got {max_seq_len}")
        dtype = self.embed_tokens.dtype
        for block in self.blocks:
            block.attn.init_fixed_cache(int(max_seq_len), dtype)
        self._decode = _DecodeBuffers(self.config, dtype)
        c = self.config
        _workspace(c.num_attention_heads, c.head_dim, int(max_seq_len))     # the attention op must not allocate under capture
        self.max_cache_len = int(max_seq_len)
        self._graph = None

    def _require_cache(self, name: str) -> _DecodeBuffers:
        if self._decode is None:
            raise RuntimeError(f"Llama4Model.{name}: call init_fixed_cache() first")
        return self._decode

    def prefill_fixed_cache(self, input_ids: np.ndarray, start_pos: int = 0) -> GPUArray:
        """input_ids [S] at positions start_pos .. start_pos+S-1 -> logits [S, vocab_size]; K / V of these rows are left
        in the caches and attention reads cache rows 0 .. start_pos+S-1, so a prompt may be fed in several chunks."""
        self._require_cache("prefill_fixed_cache")
        hidden, S = self._embed(input_ids, "prefill_fixed_cache")
        if start_pos < 0 or start_pos + S > self.max_cache_len:
            raise ValueError(f"Llama4Model.prefill_fixed_cache: rows {start_pos}..{start_pos + S} outside the cache of "
                             f"{self.max_cache_len} rows")
        positions = from_numpy(np.arange(start_pos, start_pos + S, dtype=np.int64))
        for block in self.blocks:
            hidden = block.prefill_fixed_cache(hidden, positions, int(start_pos))
        hidden = rmsnorm(hidden, self.final_norm_weight, self.config.rms_norm_eps)
        return matmul_nt(hidden, self.lm_head)

    def _set_state(self, token_id: int, position: int, name: str) -> _DecodeBuffers:
        b = self._require_cache(name)
        if not 0 <= token_id < self.embed_tokens.shape[0]:
            raise ValueError(f"Llama4Model.{name}: token id {token_id} outside [0, {self.embed_tokens.shape[0]})")
        if not 0 <= position < self.max_cache_len:
            raise ValueError(f"Llama4Model.{name}: position {position} outside the cache of {self.max_cache_len} rows")
        b.state.copy_from_numpy(np.array([token_id, position], np.int32))     # the step's only host-to-device copy
        return b

    def _decode_ops(self, b: _DecodeBuffers) -> None:
        """The one-token step on the persistent buffers: no allocation, no host value - safe to capture."""
        embedding_lookup_ptr(self.embed_tokens, b.hidden, b.token_id_buf)
        for block in self.blocks:
            block.decode_fixed_cache(b)
        rmsnorm(b.hidden, self.final_norm_weight, self.config.rms_norm_eps, out=b.normed)
        matmul_nt(b.normed, self.lm_head, out=b.logits)

    def decode_step(self, token_id: int, position: int) -> GPUArray:
        """token_id at `position` against cache rows 0 .. position-1 (its own row is written first) -> logits
        [1, vocab_size]: the model's persistent buffer, valid until the next step."""
        b = self._set_state(int(token_id), int(position), "decode_step")
        self._decode_ops(b)
        return b.logits

    def capture_decode(self) -> None:
        """Capture the whole one-token step (embedding -> every block -> final norm -> lm_head) as one graph on one stream."""
        b = self._require_cache("capture_decode")
        graph = CudaGraph()
        graph.begin_capture()
        try:
            self._decode_ops(b)
        finally:
            graph.end_capture()
        self._graph = graph

    def decode_step_graph(self, token_id: int, position: int) -> GPUArray:
        """decode_step as the 8-byte state upload + one graph replay; same logits buffer."""
        if self._graph is None:
            raise RuntimeError("Llama4Model.decode_step_graph: nothing captured for the current caches - call capture_decode() "
                               "(again after init_fixed_cache)")
        b = self._set_state(int(token_id), int(position), "decode_step_graph")
        self._graph.replay()
        return b.logits

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


def _argmax_last(logits: GPUArray) -> int:
    last = logits.to_numpy()[-1]
    if last.dtype == np.uint16:     # bfloat16 words
        last = (last.astype(np.uint32) << 16).view(np.float32)
    return int(np.argmax(last))


def generate(model: Llama4Model, input_ids: np.ndarray, max_new_tokens: int = 50, eos_token_id: int | list[int] = 200001, *,
             use_cache: bool = False, use_graph: bool = False) -> np.ndarray:
    """Greedy generation; returns the token ids including the input.  use_cache=True prefills the fixed caches (allocated
    here if the model has none with room for len(input_ids) + max_new_tokens rows) and decodes one token per step;
    use_graph=True (with use_cache) decodes through the captured step."""
    eos_token_ids = {eos_token_id} if isinstance(eos_token_id, int) else set(eos_token_id)
    current_ids = [int(t) for t in input_ids]
    if use_graph and not use_cache:
        raise ValueError("generate: use_graph=True needs use_cache=True")
    if not use_cache:
        for _ in range(max_new_tokens):
            next_token = _argmax_last(model.forward(np.array(current_ids, dtype=np.int64)))
            current_ids.append(next_token)
            if next_token in eos_token_ids:
                break
        return np.array(current_ids, dtype=np.int64)
    if max_new_tokens < 1:
        return np.array(current_ids, dtype=np.int64)
    if model.max_cache_len < len(current_ids) + max_new_tokens:
        model.init_fixed_cache(len(current_ids) + max_new_tokens)
    if use_graph and model._graph is None:
        model.capture_decode()
    step = model.decode_step_graph if use_graph else model.decode_step
    next_token = _argmax_last(model.prefill_fixed_cache(np.array(current_ids, dtype=np.int64)))
    current_ids.append(next_token)
    while len(current_ids) - len(input_ids) < max_new_tokens and next_token not in eos_token_ids:
        next_token = _argmax_last(step(next_token, len(current_ids) - 1))
        current_ids.append(next_token)
    return np.array(current_ids, dtype=np.int64)
