"""T5 text encoder (reference: src/pygpukit/diffusion/text_encoders/t5.py; the computation is HuggingFace's T5EncoderModel, v1.1).

The reference's class normalises, softmaxes and adds on the host and uploads a dense [1, H, S, S] bias for every layer.  Here the
ids are uploaded once and everything up to the result stays on the device; per batch element and layer:
    rmsnorm -> ONE q | k | v GEMM on the [3 inner, D] weight packed at load -> sdpa_relbias_strided reading that projection in place,
    the bias a [H, 2R + 1] table built once at load (ops/nn/relpos.py) -> o GEMM -> add -> rmsnorm -> ONE wi_0 | wi_1 GEMM ->
    glu_packed(gelu) -> wo GEMM -> add
inner = num_heads * d_kv is read from q.weight and need not equal hidden_size (T5-XXL: 64 * 64 = 4096 = hidden; T5 v1.1 small:
6 * 64 = 384 against 512).  Block 0's relative_attention_bias serves every layer.

Defaults are HF's: attention scale 1.0, gated gelu_new.  attention_scale=None (1 / sqrt(d_kv)) and ffn_activation="relu" give the
reference's own arithmetic.  attention_mask must be a prefix mask (ones, then zeros): element b attends its first n_b keys, which
is what the reference's -1e9 and HF's finfo.min amount to; all S query rows are computed, as both programs do.
dtype: float32 or bfloat16; float16 is accepted, but T5-XXL's FFN is known to overflow in it."""

from __future__ import annotations

import json
from pathlib import Path

import numpy as np

from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import DataType, as_dtype, float32
from pygpukit_amd.core.factory import from_numpy
from pygpukit_amd.ops.elementwise import add, mul
from pygpukit_amd.ops.embedding import embedding_lookup_batch
from pygpukit_amd.ops.matmul import matmul_nt
from pygpukit_amd.ops.nn.fused import glu_packed
from pygpukit_amd.ops.nn.norm import rmsnorm
from pygpukit_amd.ops.nn.relpos import relbias_plan, relpos_bias_table, sdpa_relbias_strided
from pygpukit_amd.ops.unary import relu

_REL = "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"


# ---- helpers shared with clip.py -------------------------------------------------------------------------------------------

def host_array(a) -> np.ndarray:
    """A weight as float32 on the host: NumPy arrays as they are, GPUArrays downloaded (bfloat16 words widened)."""
    if isinstance(a, GPUArray):
        a = a.astype(float32).to_numpy() if a.dtype.name in ("float16", "bfloat16") else a.to_numpy()
    return np.asarray(a, dtype=np.float32)


def to_device(a, dtype: DataType) -> GPUArray:
    return from_numpy(np.ascontiguousarray(host_array(a), dtype=np.float32)).astype(dtype)


def load_tokenizer(tokenizer):
    """None, a tokenizers.Tokenizer, or the path of a tokenizer.json (or of the directory that holds one)."""
    if tokenizer is None or hasattr(tokenizer, "encode_batch"):
        return tokenizer
    from tokenizers import Tokenizer

    path = Path(tokenizer)
    if path.is_dir():
        path = path / "tokenizer.json"
    return Tokenizer.from_file(str(path))


def tokenize_with(tokenizer, text, max_length: int, padding: bool, truncation: bool, fallback):
    """The reference's tokenize(): (ids, mask) int64 [B, max_length] on the HOST (the reference uploads them; forward does that here).
    fallback(text) -> ids of one string when there is no tokenizer."""
    texts = [text] if isinstance(text, str) else list(text)
    if tokenizer is not None:
        rows = [list(enc.ids) for enc in tokenizer.encode_batch(texts)]
    else:
        rows = [fallback(t) for t in texts]
        padding = truncation = True
    if truncation:
        rows = [r[:max_length] for r in rows]
    width = max_length if padding else max(len(r) for r in rows)
    ids = np.zeros((len(rows), width), np.int64)
    mask = np.zeros((len(rows), width), np.int64)
    for i, r in enumerate(rows):
        ids[i, :len(r)] = r
        mask[i, :len(r)] = 1
    return ids, mask


def prefix_lengths(attention_mask, batch: int, seq: int) -> list[int]:
    """Valid tokens per element of a prefix mask [B, S] (ones, then zeros, at least one 1); anything else is a ValueError."""
    if attention_mask is None:
        return [seq] * batch
    m = attention_mask.to_numpy() if isinstance(attention_mask, GPUArray) else np.asarray(attention_mask)
    m = m.reshape(1, -1) if m.ndim == 1 else m
    if m.shape != (batch, seq):
        raise ValueError(f"attention_mask must be [{batch}, {seq}], got {m.shape}")
    if not np.isin(m, (0, 1)).all():
        raise ValueError("attention_mask must hold zeros and ones")
    n = m.sum(axis=1).astype(np.int64)
    if (n < 1).any() or (m != (np.arange(seq)[None, :] < n[:, None])).any():
        raise ValueError("attention_mask must be a prefix mask: ones, then zeros, with at least one 1 in every row (a hole or a "
                         "left-padded row cannot be expressed as a key count)")
    return [int(x) for x in n]


def ids_on_host(input_ids) -> np.ndarray:
    ids = input_ids.to_numpy() if isinstance(input_ids, GPUArray) else np.asarray(input_ids)
    ids = ids.reshape(1, -1) if ids.ndim == 1 else ids
    if ids.ndim != 2 or ids.shape[1] < 1 or not np.issubdtype(ids.dtype, np.integer):
        raise ValueError(f"input_ids must be integers [B, seq], got {ids.dtype} {ids.shape}")
    return ids


class SafetensorsWeights:
    """{name: float32 array} view of a safetensors file or sharded index, read tensor by tensor (a T5-XXL does not fit the host twice)."""

    def __init__(self, path, single_names):
        from pygpukit_amd.llm.safetensors import load_safetensors

        path = Path(path)
        base = path if path.is_dir() else path.parent
        if path.is_dir() or path.name.endswith(".index.json"):
            index = path if not path.is_dir() else next((base / n for n in ("model.safetensors.index.fp16.json", "model.safetensors.index.json")
                                                         if (base / n).exists()), None)
            if index is None:
                found = next((base / n for n in single_names if (base / n).exists()), None)
                if found is None:
                    raise FileNotFoundError(f"no safetensors file ({', '.join(single_names)}) or index in {base}")
                path = found
            else:
                path = index
        self.base = base
        self._st = load_safetensors(str(path))
        self._names = set(self._st.tensor_names)

    def keys(self):
        return self._names

    def __contains__(self, name) -> bool:
        return name in self._names

    def __getitem__(self, name) -> np.ndarray:
        return self._st.tensor_as_f32(name)

    def get(self, name, default=None):
        return self[name] if name in self._names else default

    def shape(self, name):
        return tuple(self._st.tensor_info(name).shape)

    def find_tokenizer(self):
        for p in (self.base / "tokenizer.json", self.base.parent / "tokenizer" / "tokenizer.json", self.base.parent / "tokenizer_2" / "tokenizer.json"):
            if p.exists():
                return str(p)
        return None


# ---- the encoder -----------------------------------------------------------------------------------------------------------

def t5_plan(hidden_size: int, num_heads: int, d_kv: int, d_ff: int, seq_len: int, dtype="float32", ffn_activation: str = "gelu",
            max_distance: int = 128) -> dict:
    """Host-only: op launches per layer and element (attention counted as one op: its flash path adds a V-transpose pre-pass and, for
    short prompts, a merge of the KV runs) and the attention kernel sdpa_relbias takes."""
    return {"launches_per_layer": 10 if ffn_activation == "gelu" else 12,
            "attention": relbias_plan(d_kv, max_distance, dtype, aligned=(num_heads * d_kv) % 8 == 0 and d_kv % 8 == 0),
            "table_bytes": num_heads * (2 * max_distance + 1) * 4, "dense_bias_bytes": num_heads * seq_len * seq_len * 4}


class _T5Layer:
    __slots__ = ("ln0", "qkv", "o", "ln1", "wi", "wi0", "wi1", "wo")


class T5Encoder:
    """T5 encoder for diffusion pipelines (SD3, FLUX): forward(input_ids, attention_mask) -> hidden states [B, seq, hidden_size]."""

    def __init__(self, hidden_size: int = 4096, num_layers: int = 24, num_heads: int = 64, d_ff: int = 10240, max_length: int = 512,
                 weights: "dict | None" = None, *, dtype: "str | DataType" = "float32", tokenizer=None, attention_scale: "float | None" = 1.0,
                 ffn_activation: str = "gelu", max_distance: int = 128, eps: float = 1e-6):
        if ffn_activation not in ("gelu", "relu"):
            raise ValueError(f"T5Encoder: ffn_activation must be 'gelu' (HF's gated gelu_new) or 'relu' (the reference's gate), got {ffn_activation!r}")
        self.hidden_size, self.num_layers, self.num_heads, self.d_ff, self.max_length = hidden_size, num_layers, num_heads, d_ff, max_length
        self.dtype = as_dtype(dtype)
        self.attention_scale = None if attention_scale is None else float(attention_scale)
        self.ffn_activation = ffn_activation
        self.max_distance, self.eps = int(max_distance), float(eps)
        self.tokenizer = load_tokenizer(tokenizer)
        self.weights = weights if weights is not None else {}
        self.layers: list[_T5Layer] = []
        self.inner = self.d_kv = 0
        if weights:
            self._load(weights)

    # ------------------------------------------------------------------ loading
    def _load(self, w) -> None:
        dt = self.dtype
        name = "shared.weight" if "shared.weight" in w else "encoder.embed_tokens.weight"
        self.embed = to_device(w[name], dt)
        if self.embed.shape[1] != self.hidden_size:
            raise ValueError(f"T5Encoder: embedding width {self.embed.shape[1]} is not hidden_size {self.hidden_size}")
        rel = host_array(w[_REL])
        if rel.shape[1] != self.num_heads:
            raise ValueError(f"T5Encoder: relative_attention_bias has {rel.shape[1]} heads, expected {self.num_heads}")
        self.num_buckets = rel.shape[0]
        self.bias_table = relpos_bias_table(rel, True, self.max_distance)          # [H, 2R + 1] float32, once
        for i in range(self.num_layers):
            p, L = f"encoder.block.{i}.layer", _T5Layer()
            q, k, v = (host_array(w[f"{p}.0.SelfAttention.{n}.weight"]) for n in "qkv")
            if i == 0:
                self.inner = q.shape[0]
                if self.inner % self.num_heads:
                    raise ValueError(f"T5Encoder: q.weight has {self.inner} rows, no multiple of {self.num_heads} heads")
                self.d_kv = self.inner // self.num_heads
            L.qkv = to_device(np.concatenate([q, k, v], axis=0), dt)
            L.o = to_device(w[f"{p}.0.SelfAttention.o.weight"], dt)
            L.ln0, L.ln1 = to_device(w[f"{p}.0.layer_norm.weight"], dt), to_device(w[f"{p}.1.layer_norm.weight"], dt)
            wi0, wi1 = (host_array(w[f"{p}.1.DenseReluDense.{n}.weight"]) for n in ("wi_0", "wi_1"))
            if wi0.shape[0] != self.d_ff:
                raise ValueError(f"T5Encoder: wi_0 has {wi0.shape[0]} rows, expected d_ff {self.d_ff}")
            L.wi = L.wi0 = L.wi1 = None
            if self.ffn_activation == "gelu":
                L.wi = to_device(np.concatenate([wi0, wi1], axis=0), dt)
            else:
                L.wi0, L.wi1 = to_device(wi0, dt), to_device(wi1, dt)
            L.wo = to_device(w[f"{p}.1.DenseReluDense.wo.weight"], dt)
            self.layers.append(L)
        self.final_ln = to_device(w["encoder.final_layer_norm.weight"], dt)

    @classmethod
    def from_safetensors(cls, path, dtype: "str | DataType" = "float32", **kwargs) -> "T5Encoder":
        """A file, a sharded index or a directory (model.safetensors[.index.json], text_encoder_2.safetensors); the sizes are read
        from the tensors and tokenizer.json is picked up when it lies beside them."""
        w = SafetensorsWeights(path, ("model.safetensors", "text_encoder_2.safetensors"))
        embed = "shared.weight" if "shared.weight" in w else "encoder.embed_tokens.weight"
        blocks = {int(n.split("block.")[1].split(".")[0]) for n in w.keys() if "encoder.block." in n}
        kwargs.setdefault("tokenizer", w.find_tokenizer())
        return cls(hidden_size=w.shape(embed)[1], num_layers=max(blocks) + 1, num_heads=w.shape(_REL)[1],
                   d_ff=w.shape("encoder.block.0.layer.1.DenseReluDense.wi_0.weight")[0], weights=w, dtype=dtype, **kwargs)

    # ------------------------------------------------------------------ text
    def tokenize(self, text, max_length: "int | None" = None, padding: bool = True, truncation: bool = True):
        """(input_ids, attention_mask), int64 [B, max_length] on the host.  Without a tokenizer: the reference's fallback,
        ord(c) % 32000 per character and EOS 1."""
        max_length = self.max_length if max_length is None else int(max_length)
        return tokenize_with(self.tokenizer, text, max_length, padding, truncation,
                             lambda t: [ord(c) % 32000 for c in t][:max_length - 1] + [1])

    def encode(self, text) -> GPUArray:
        return self.forward(*self.tokenize(text))

    # ------------------------------------------------------------------ forward
    def plan(self, seq_len: int) -> dict:
        return t5_plan(self.hidden_size, self.num_heads, self.d_kv, self.d_ff, seq_len, self.dtype, self.ffn_activation, self.max_distance)

    def _layer(self, L: _T5Layer, x: GPUArray, n_valid: int) -> GPUArray:
        S, H, dk, inner = x.shape[0], self.num_heads, self.d_kv, self.inner
        qkv = matmul_nt(rmsnorm(x, L.ln0, self.eps), L.qkv)                       # [S, 3 inner]: q | k | v per row
        rest = qkv.size - 2 * inner
        attn = GPUArray((S, inner), self.dtype)
        sdpa_relbias_strided(qkv, qkv._view(inner, (rest,)), qkv._view(2 * inner, (rest,)), self.bias_table, attn, H, H, S, n_valid, dk,
                             (dk, 3 * inner), (dk, 3 * inner), (dk, inner), 0.0 if self.attention_scale is None else self.attention_scale)
        x = add(x, matmul_nt(attn, L.o))
        h = rmsnorm(x, L.ln1, self.eps)
        if L.wi is not None:
            g = glu_packed(matmul_nt(h, L.wi), self.d_ff, activation="gelu")
        else:
            g = mul(relu(matmul_nt(h, L.wi0)), matmul_nt(h, L.wi1))
        return add(x, matmul_nt(g, L.wo))

    def forward(self, input_ids, attention_mask=None) -> GPUArray:
        if not self.layers:
            raise RuntimeError("T5Encoder.forward: no weights were given")
        if self.attention_scale is not None and not self.attention_scale > 0:
            raise ValueError(f"T5Encoder: attention_scale must be positive or None, got {self.attention_scale}")
        ids = ids_on_host(input_ids)
        B, S = ids.shape
        if ids.min() < 0 or ids.max() >= self.embed.shape[0]:
            raise ValueError(f"T5Encoder: token ids outside [0, {self.embed.shape[0]})")
        valid = prefix_lengths(attention_mask, B, S)
        ids_dev = from_numpy(np.ascontiguousarray(ids, dtype=np.int32))
        D = self.hidden_size
        out = GPUArray((B, S, D), self.dtype)
        for b in range(B):
            x = GPUArray((S, D), self.dtype)
            embedding_lookup_batch(self.embed, x, ids_dev._view(b * S, (S,)), S)
            for L in self.layers:
                x = self._layer(L, x, valid[b])
            rmsnorm(x, self.final_ln, self.eps, out=out._view(b * S * D, (S, D)))
        return out

    __call__ = forward


class T5XXLEncoder(T5Encoder):
    """T5-XXL (4096 wide, 24 layers, 64 heads of 64, d_ff 10240): SD3's and FLUX's second text encoder."""

    def __init__(self, **kwargs):
        kwargs.setdefault("hidden_size", 4096)
        kwargs.setdefault("num_layers", 24)
        kwargs.setdefault("num_heads", 64)
        kwargs.setdefault("d_ff", 10240)
        kwargs.setdefault("max_length", 512)
        super().__init__(**kwargs)


__all__ = ["T5Encoder", "T5XXLEncoder", "t5_plan"]
