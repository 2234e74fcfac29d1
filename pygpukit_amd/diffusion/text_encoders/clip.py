"""CLIP text encoder (reference: src/pygpukit/diffusion/text_encoders/clip.py, whose layers are a stub: "attention" is a mean over
the tokens and the learned weights are never read).  The computation here is HuggingFace's CLIPTextModel, built from existing ops:
token + position embedding (gathered on the device), pre-LN blocks - layernorm, ONE biased q | k | v GEMM on the weight packed at
load, sdpa_causal_strided reading it in place (head_dim 64: the MFMA flash kernels in the 16-bit dtypes), out_proj, add, layernorm,
fc1, quick_gelu or gelu, fc2, add - and the final LayerNorm.

Pooled output: the final-norm row at the first eos_token_id (argmax of the ids when eos_token_id == 2, HF's rule for old configs),
found on the host - not the reference's last row x[:, -1].  With text_projection.weight present (CLIP-G's WithProjection form) the
pooled row goes through it.  attention_mask is accepted and ignored, as in the reference's class: under the causal mask no row up to
the EOS can see the padding after it, so the pooled output cannot depend on it (rows after the EOS do attend the padding, as in
diffusers' pipelines, which pass no mask either).  hidden_act "gelu" is the tanh form of the gelu op (HF's is the erf form; they
differ by less than 5e-4 in absolute value).  Weight names are accepted with and without the text_model. prefix.

The residual stream is float32 in every dtype: in a 16-bit model the GEMMs, the attention and the activation run in the model's
dtype, each sublayer's output is widened and added to the float32 stream, and each LayerNorm reads the stream and hands its result
on in the model's dtype (its weights and the embeddings hold the dtype's values).  Rounding the stream to bfloat16 after every add
is the largest single share of a bfloat16 model's error (about a third of it on the test fixture), for four casts per layer."""

from __future__ import annotations

import numpy as np

from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import DataType, as_dtype, float32
from pygpukit_amd.core.factory import from_numpy
from pygpukit_amd.diffusion.text_encoders.t5 import SafetensorsWeights, host_array, ids_on_host, load_tokenizer, to_device, tokenize_with
from pygpukit_amd.ops.elementwise import add, copy_to
from pygpukit_amd.ops.embedding import embedding_lookup_batch
from pygpukit_amd.ops.matmul import matmul_nt
from pygpukit_amd.ops.nn.activation import gelu, quick_gelu
from pygpukit_amd.ops.nn.attention import sdpa_causal_strided
from pygpukit_amd.ops.nn.norm import layernorm

_PREFIX = "text_model."
_ACTS = {"quick_gelu": quick_gelu, "gelu": gelu}


def pooled_position(ids_row, eos_token_id: int) -> int:
    """HF's rule: argmax of the ids when eos_token_id == 2, else the first position that holds eos_token_id (0 when none does)."""
    ids_row = np.asarray(ids_row)
    if eos_token_id == 2:
        return int(np.argmax(ids_row))
    return int(np.argmax(ids_row == eos_token_id))


class _Weights:
    """Names with or without the text_model. prefix (transformers 5 state dicts drop it; checkpoints on disk carry it)."""

    def __init__(self, w):
        self.w = w

    def _name(self, name):
        for n in (_PREFIX + name, name):
            if n in self.w:
                return n
        return None

    def __contains__(self, name) -> bool:
        return self._name(name) is not None

    def __getitem__(self, name):
        n = self._name(name)
        if n is None:
            raise KeyError(f"CLIPTextEncoder: weight {name!r} not found (with or without the {_PREFIX!r} prefix)")
        return self.w[n]


class _ClipLayer:
    __slots__ = ("ln1", "qkv_w", "qkv_b", "out_w", "out_b", "ln2", "fc1_w", "fc1_b", "fc2_w", "fc2_b")


class CLIPTextEncoder:
    """forward(input_ids) -> (last_hidden_state [B, seq, hidden], pooled [B, hidden or projection_dim])."""

    def __init__(self, hidden_size: int = 768, num_layers: int = 12, num_heads: int = 12, max_length: int = 77, weights: "dict | None" = None,
                 *, dtype: "str | DataType" = "float32", tokenizer=None, hidden_act: str = "quick_gelu", eos_token_id: int = 49407,
                 eps: float = 1e-5):
        if hidden_act not in _ACTS:
            raise ValueError(f"CLIPTextEncoder: hidden_act must be one of {sorted(_ACTS)}, got {hidden_act!r}")
        if hidden_size % num_heads:
            raise ValueError(f"CLIPTextEncoder: hidden_size {hidden_size} is no multiple of {num_heads} heads")
        self.hidden_size, self.num_layers, self.num_heads, self.max_length = hidden_size, num_layers, num_heads, max_length
        self.head_dim = hidden_size // num_heads
        self.dtype = as_dtype(dtype)
        self.hidden_act, self.eos_token_id, self.eps = hidden_act, int(eos_token_id), float(eps)
        self.tokenizer = load_tokenizer(tokenizer)
        self.weights = weights if weights is not None else {}
        self.layers: list[_ClipLayer] = []
        self.text_projection = None
        if weights:
            self._load(_Weights(weights))

    def _load(self, w: _Weights) -> None:
        dt = self.dtype

        def pair(name):
            return to_device(w[name + ".weight"], dt), to_device(w[name + ".bias"], dt)

        def norm(name):      # LayerNorm reads the float32 stream: the dtype's values, held as float32
            return tuple(a.astype(float32) for a in pair(name))

        self.token_embedding = to_device(w["embeddings.token_embedding.weight"], dt)
        self.position_embedding = to_device(w["embeddings.position_embedding.weight"], dt).astype(float32)
        if self.token_embedding.shape[1] != self.hidden_size:
            raise ValueError(f"CLIPTextEncoder: embedding width {self.token_embedding.shape[1]} is not hidden_size {self.hidden_size}")
        for i in range(self.num_layers):
            p, L = f"encoder.layers.{i}.", _ClipLayer()
            L.ln1, L.ln2 = norm(p + "layer_norm1"), norm(p + "layer_norm2")
            L.qkv_w = to_device(np.concatenate([host_array(w[f"{p}self_attn.{n}.weight"]) for n in ("q_proj", "k_proj", "v_proj")], axis=0), dt)
            L.qkv_b = to_device(np.concatenate([host_array(w[f"{p}self_attn.{n}.bias"]) for n in ("q_proj", "k_proj", "v_proj")]), dt)
            L.out_w, L.out_b = pair(p + "self_attn.out_proj")
            L.fc1_w, L.fc1_b = pair(p + "mlp.fc1")
            L.fc2_w, L.fc2_b = pair(p + "mlp.fc2")
            self.layers.append(L)
        self.final_ln = norm("final_layer_norm")
        if "text_projection.weight" in w.w:
            self.text_projection = to_device(w.w["text_projection.weight"], dt)

    @classmethod
    def from_safetensors(cls, path, dtype: "str | DataType" = "float32", **kwargs) -> "CLIPTextEncoder":
        """A file or a directory (model.safetensors, text_encoder.safetensors); sizes are read from the tensors (head_dim 64, as
        in every released CLIP text tower, unless num_heads= is given) and tokenizer.json is picked up when it lies beside them."""
        st = SafetensorsWeights(path, ("model.safetensors", "text_encoder.safetensors"))
        w = _Weights(st)
        embed = w._name("embeddings.token_embedding.weight")
        if embed is None:
            raise KeyError("CLIPTextEncoder.from_safetensors: embeddings.token_embedding.weight not found")
        hidden = st.shape(embed)[1]
        layers = {int(n.split("encoder.layers.")[1].split(".")[0]) for n in st.keys() if "encoder.layers." in n}
        kwargs.setdefault("num_heads", max(1, hidden // 64))
        kwargs.setdefault("tokenizer", st.find_tokenizer())
        kwargs.setdefault("max_length", st.shape(w._name("embeddings.position_embedding.weight"))[0])
        return cls(hidden_size=hidden, num_layers=max(layers) + 1, weights=st, dtype=dtype, **kwargs)

    # ------------------------------------------------------------------ text
    def tokenize(self, text, max_length: "int | None" = None, padding: bool = True, truncation: bool = True):
        """(input_ids, attention_mask), int64 [B, max_length] on the host.  Without a tokenizer: the reference's fallback,
        BOS 49406, ord(c) % 10000 per character, EOS 49407."""
        max_length = self.max_length if max_length is None else int(max_length)
        return tokenize_with(self.tokenizer, text, max_length, padding, truncation,
                             lambda t: [49406] + [ord(c) % 10000 for c in t][:max_length - 2] + [49407])

    def encode(self, text, output_hidden_states: bool = False):
        return self.forward(*self.tokenize(text))

    # ------------------------------------------------------------------ forward
    def _layer(self, L: _ClipLayer, x: GPUArray) -> GPUArray:
        """x: the float32 residual stream [S, d]; astype is the identity in a float32 model."""
        S, d, H, hd = x.shape[0], self.hidden_size, self.num_heads, self.head_dim
        qkv = matmul_nt(layernorm(x, *L.ln1, self.eps).astype(self.dtype), L.qkv_w, L.qkv_b)         # [S, 3 d]: q | k | v per row
        rest = qkv.size - 2 * d
        attn = GPUArray((S, d), self.dtype)
        sdpa_causal_strided(qkv, qkv._view(d, (rest,)), qkv._view(2 * d, (rest,)), attn, H, H, S, S, hd, (hd, 3 * d), (hd, 3 * d), (hd, d))
        x = add(x, matmul_nt(attn, L.out_w, L.out_b).astype(float32))
        f = matmul_nt(layernorm(x, *L.ln2, self.eps).astype(self.dtype), L.fc1_w, L.fc1_b)
        _ACTS[self.hidden_act](f, out=f)
        return add(x, matmul_nt(f, L.fc2_w, L.fc2_b).astype(float32))

    def forward(self, input_ids, attention_mask=None):
        if not self.layers:
            raise RuntimeError("CLIPTextEncoder.forward: no weights were given")
        ids = ids_on_host(input_ids)
        B, S = ids.shape
        if S > self.position_embedding.shape[0]:
            raise ValueError(f"CLIPTextEncoder: {S} tokens, {self.position_embedding.shape[0]} positions")
        if ids.min() < 0 or ids.max() >= self.token_embedding.shape[0]:
            raise ValueError(f"CLIPTextEncoder: token ids outside [0, {self.token_embedding.shape[0]})")
        ids_dev = from_numpy(np.ascontiguousarray(ids, dtype=np.int32))
        d = self.hidden_size
        pos = self.position_embedding._view(0, (S, d))
        hidden = GPUArray((B, S, d), self.dtype)
        pooled = GPUArray((B, d), self.dtype)
        for b in range(B):
            tok = GPUArray((S, d), self.dtype)
            embedding_lookup_batch(self.token_embedding, tok, ids_dev._view(b * S, (S,)), S)
            x = add(tok.astype(float32), pos)
            for L in self.layers:
                x = self._layer(L, x)
            if self.dtype == float32:
                layernorm(x, *self.final_ln, self.eps, out=hidden._view(b * S * d, (S, d)))
            else:
                copy_to(layernorm(x, *self.final_ln, self.eps).astype(self.dtype), hidden._view(b * S * d, (S, d)))
            at = pooled_position(ids[b], self.eos_token_id)
            copy_to(hidden._view((b * S + at) * d, (1, d)), pooled._view(b * d, (1, d)))
        if self.text_projection is not None:
            pooled = matmul_nt(pooled, self.text_projection)
        return hidden, pooled

    __call__ = forward


class CLIPTextEncoderL(CLIPTextEncoder):
    """CLIP-L text tower (768 wide, 12 layers, 12 heads, quick_gelu)."""

    def __init__(self, **kwargs):
        kwargs.setdefault("hidden_size", 768)
        kwargs.setdefault("num_layers", 12)
        kwargs.setdefault("num_heads", 12)
        super().__init__(**kwargs)


class CLIPTextEncoderG(CLIPTextEncoder):
    """CLIP-G text tower (1280 wide, 32 layers, 20 heads, gelu, text_projection)."""

    def __init__(self, **kwargs):
        kwargs.setdefault("hidden_size", 1280)
        kwargs.setdefault("num_layers", 32)
        kwargs.setdefault("num_heads", 20)
        kwargs.setdefault("hidden_act", "gelu")
        super().__init__(**kwargs)


__all__ = ["CLIPTextEncoder", "CLIPTextEncoderL", "CLIPTextEncoderG", "pooled_position"]
