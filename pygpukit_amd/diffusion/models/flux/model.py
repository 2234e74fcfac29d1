"""FLUX.1 transformer (reference: src/pygpukit/diffusion/models/flux/model.py, blocks.py, attention.py).  The computation is the
reference's, quirks included (INTEGRATION.md "FLUX transformer"); the reference runs LayerNorm, every modulation and every
residual on the host in NumPy with a to_numpy() round trip between them - here a step stays on the device:

  * modulations: every norm1.linear / norm1_context.linear / norm.linear / norm_out.linear weight and bias is packed at load time
    into ONE matrix of (12 L + 3 Ls + 2) D rows; a step runs one silu and one matmul_nt on temb and every block reads its vectors
    in place (diffusion.ops.Modulation over the projection).  No second copy of those weights is kept.
  * the residual stream lives in one joint [T + I, D] buffer (text rows first), so the double blocks' two streams are row ranges
    of it and the single blocks need no concatenation;
  * double block, 16 launches: two fused q|k|v GEMMs writing the text and the image rows of one [T + I, 3 D] buffer, ONE
    flux_qk_norm_rope (split = T: norm_added_* for the text rows, norm_* for the image rows), ONE sdpa_noncausal_strided reading
    the projection in place, two out projections, and per stream gated_residual_adaln twice (attention residual + modulated
    norm2; FFN residual + the NEXT block's modulated norm1) around linear_bias_gelu + GEMM;
  * single block, 7 launches: q|k|v GEMM, proj_mlp GEMM, flux_qk_norm_rope, attention writing columns 0..D of the [S, 5 D]
    operand of proj_out, flux_gelu_pack writing columns D..5 D, the proj_out GEMM, gated_residual_adaln;
  * set_encoder_states runs context_embedder and the pooled text_embedder MLP once per prompt; the RoPE tables are cached per ids.
Batch elements are run one after another through the block stack (the GEMM outputs and the attention call are per element), each
with its own conditioning row; the conditioning path and the modulation GEMM run once for the whole batch."""

from __future__ import annotations

import os
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import DataType, as_dtype, float32
from pygpukit_amd.core.factory import from_numpy
from pygpukit_amd.diffusion.models.flux.embeddings import (get_rope_frequencies, prepare_image_ids, prepare_text_ids,
                                                           timestep_embedding)
from pygpukit_amd.diffusion.ops.adaln import Modulation, gated_residual, gated_residual_adaln
from pygpukit_amd.diffusion.ops.flux import flux_gelu_pack, flux_qk_norm_rope, flux_qk_norm_rope_plan
from pygpukit_amd.ops.elementwise import add, copy_to
from pygpukit_amd.ops.matmul import linear_bias_gelu, matmul_nt
from pygpukit_amd.ops.nn.activation import silu
from pygpukit_amd.ops.nn.attention import sdpa_noncausal_strided

EPS = 1e-6               # LayerNorm and the per-head RMSNorm, as the reference
TIME_EMBED_DIM = 256
LAUNCHES_DOUBLE = 16
LAUNCHES_SINGLE = 7


@dataclass
class FluxConfig:
    in_channels: int = 64
    out_channels: "int | None" = None
    hidden_size: int = 3072
    num_layers: int = 19
    num_single_layers: int = 38
    num_attention_heads: int = 24
    attention_head_dim: int = 128
    joint_attention_dim: int = 4096
    pooled_projection_dim: int = 768
    guidance_embeds: bool = False
    axes_dims_rope: "tuple[int, int, int]" = (16, 56, 56)

    @property
    def head_dim(self) -> int:
        return self.attention_head_dim


def modulation_layout(config: FluxConfig) -> dict:
    """Row offsets (in units of rows of the packed modulation matrix) of every block's vectors:
    {"double": [(norm1, norm1_context)], "single": [norm], "out": norm_out, "rows": total}.  A double block's 6 D rows are shift_msa,
    scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp; a single block's 3 D are shift, scale, gate; norm_out's 2 D are scale, shift."""
    D, L, Ls = config.hidden_size, config.num_layers, config.num_single_layers
    return {"double": [(12 * D * i, 12 * D * i + 6 * D) for i in range(L)],
            "single": [12 * D * L + 3 * D * j for j in range(Ls)],
            "out": (12 * L + 3 * Ls) * D, "rows": (12 * L + 3 * Ls + 2) * D}


def modulation_names(config: FluxConfig) -> "list[str]":
    """The linear layers whose weights make up the packed matrix, in row order."""
    names = []
    for i in range(config.num_layers):
        names += [f"transformer_blocks.{i}.norm1.linear", f"transformer_blocks.{i}.norm1_context.linear"]
    names += [f"single_transformer_blocks.{j}.norm.linear" for j in range(config.num_single_layers)]
    return names + ["norm_out.linear"]


def pack_qkv(weights: dict, prefix: str, names=("to_q", "to_k", "to_v"), suffix: str = "weight") -> np.ndarray:
    """q rows, then k rows, then v rows: the fused projection's output row is q | k | v."""
    return np.concatenate([np.asarray(weights[f"{prefix}.{n}.{suffix}"], np.float32) for n in names], axis=0)


def flux_plan(config: FluxConfig, dtype="float32", batch: int = 1) -> dict:
    """What a step runs: {"attention": "flash" | "fallback", "qk_norm_rope": the kernel flux_qk_norm_rope takes on the fused
    projection, "launches_double", "launches_single", "launches_step"}.  launches_step counts every kernel launch of
    forward(hidden_states, timestep=...) after set_encoder_states, with hidden_states in the model dtype and the RoPE tables
    cached: the conditioning path (timestep MLP 3, + pooled embedding 1, guidance 4 more, silu 1, a cast unless float32, the
    modulation GEMM 1), then per batch element x_embedder 1, the text rows' copy 1, the first modulated norms 2, the blocks and
    proj_out 1."""
    dt = as_dtype(dtype)
    hd, D = config.head_dim, config.hidden_size
    flash_on = os.environ.get("PYGPUKIT_FLASH_ATTENTION") not in ("0", "false")
    flash = dt != float32 and hd in (64, 128) and flash_on
    aligned = (hd * dt.itemsize) % 16 == 0 and (3 * D * dt.itemsize) % 16 == 0 and (config.num_attention_heads * hd * dt.itemsize) % 16 == 0
    cond = 3 + 1 + (4 if config.guidance_embeds else 0) + 1 + (0 if dt == float32 else 1) + 1
    per_element = 1 + 1 + 2 + LAUNCHES_DOUBLE * config.num_layers + LAUNCHES_SINGLE * config.num_single_layers + 1
    return {"attention": "flash" if flash else "fallback", "qk_norm_rope": flux_qk_norm_rope_plan(hd, dt, aligned),
            "launches_double": LAUNCHES_DOUBLE, "launches_single": LAUNCHES_SINGLE, "launches_step": cond + batch * per_element}


def _host(a) -> np.ndarray:
    if isinstance(a, GPUArray):
        a = a.astype(float32).to_numpy()
    return np.ascontiguousarray(a, dtype=np.float32)


class _Double:
    __slots__ = ("qkv_w", "qkv_b", "add_qkv_w", "add_qkv_b", "out_w", "out_b", "add_out_w", "add_out_b", "norm_q", "norm_k",
                 "norm_added_q", "norm_added_k", "ff1_w", "ff1_b", "ff2_w", "ff2_b", "ffc1_w", "ffc1_b", "ffc2_w", "ffc2_b")


class _Single:
    __slots__ = ("qkv_w", "qkv_b", "mlp_w", "mlp_b", "out_w", "out_b", "norm_q", "norm_k")


class FluxTransformer:
    """forward(hidden_states [B, I, in_channels], encoder_hidden_states [B, T, joint_attention_dim], pooled_projections
    [B, pooled_projection_dim], timestep [B]) -> [B, I, out_channels] in `dtype`."""

    def __init__(self, config: FluxConfig, weights: dict, dtype: "str | DataType" = "float32"):
        self.config = config
        self.dtype = as_dtype(dtype)
        self.hidden_size = D = config.hidden_size
        self.num_heads = H = config.num_attention_heads
        self.head_dim = hd = config.head_dim
        if H * hd != D:
            raise ValueError(f"FluxTransformer: hidden_size {D} is not {H} heads of {hd}")
        if sum(config.axes_dims_rope) != hd:
            raise ValueError(f"FluxTransformer: axes_dims_rope {config.axes_dims_rope} does not sum to head_dim {hd}")
        self.out_channels = config.out_channels or config.in_channels
        self.plan = flux_plan(config, self.dtype)
        self.attn_scale = 1.0 / float(np.sqrt(hd))

        def get(name):
            if name not in weights:
                raise KeyError(f"FluxTransformer: missing tensor {name}")
            return _host(weights[name])

        def bias(name, rows):
            return _host(weights[name]) if name in weights else np.zeros(rows, np.float32)

        def dev(a, dt=None):
            return from_numpy(np.ascontiguousarray(a, dtype=np.float32)).astype(dt or self.dtype)

        def lin(name, dt=None):
            w = get(name + ".weight")
            return dev(w, dt), dev(bias(name + ".bias", w.shape[0]), dt)

        def fused(prefix, names):
            ws = [get(f"{prefix}.{n}.weight") for n in names]
            return dev(np.concatenate(ws)), dev(np.concatenate([bias(f"{prefix}.{n}.bias", w.shape[0]) for n, w in zip(names, ws)]))

        self.x_w, self.x_b = lin("x_embedder")
        self.ctx_w, self.ctx_b = lin("context_embedder")
        self.proj_w, self.proj_b = lin("proj_out")
        if self.x_w.shape != (D, config.in_channels) or self.proj_w.shape != (self.out_channels, D):
            raise ValueError(f"FluxTransformer: x_embedder {self.x_w.shape} / proj_out {self.proj_w.shape} do not fit the config")
        # the conditioning path stays float32 whatever the dtype: three tiny MLPs on [B, 256] / [B, pooled] rows
        te = "time_text_embed."
        self.t1_w, self.t1_b = lin(te + "timestep_embedder.linear_1", float32)
        self.t2_w, self.t2_b = lin(te + "timestep_embedder.linear_2", float32)
        self.p1_w, self.p1_b = lin(te + "text_embedder.linear_1", float32)
        self.p2_w, self.p2_b = lin(te + "text_embedder.linear_2", float32)
        if config.guidance_embeds:
            self.g1_w, self.g1_b = lin(te + "guidance_embedder.linear_1", float32)
            self.g2_w, self.g2_b = lin(te + "guidance_embedder.linear_2", float32)
        self.layout = modulation_layout(config)
        names = modulation_names(config)
        self.mod_w = dev(np.concatenate([get(n + ".weight") for n in names]))
        self.mod_b = dev(np.concatenate([bias(n + ".bias", get(n + ".weight").shape[0]) for n in names]))
        if self.mod_w.shape != (self.layout["rows"], D):
            raise ValueError(f"FluxTransformer: the modulation weights stack to {self.mod_w.shape}, expected {(self.layout['rows'], D)}")

        self.double, self.single = [], []
        for i in range(config.num_layers):
            p, b = f"transformer_blocks.{i}", _Double()
            b.qkv_w, b.qkv_b = fused(p + ".attn", ("to_q", "to_k", "to_v"))
            b.add_qkv_w, b.add_qkv_b = fused(p + ".attn", ("add_q_proj", "add_k_proj", "add_v_proj"))
            b.out_w, b.out_b = lin(p + ".attn.to_out.0")
            b.add_out_w, b.add_out_b = lin(p + ".attn.to_add_out")
            for n in ("norm_q", "norm_k", "norm_added_q", "norm_added_k"):
                setattr(b, n, dev(get(f"{p}.attn.{n}.weight"), float32))
            b.ff1_w, b.ff1_b = lin(p + ".ff.net.0.proj")
            b.ff2_w, b.ff2_b = lin(p + ".ff.net.2")
            b.ffc1_w, b.ffc1_b = lin(p + ".ff_context.net.0.proj")
            b.ffc2_w, b.ffc2_b = lin(p + ".ff_context.net.2")
            self.double.append(b)
        for j in range(config.num_single_layers):
            p, s = f"single_transformer_blocks.{j}", _Single()
            s.qkv_w, s.qkv_b = fused(p + ".attn", ("to_q", "to_k", "to_v"))
            s.mlp_w, s.mlp_b = lin(p + ".proj_mlp")
            s.out_w, s.out_b = lin(p + ".proj_out")
            s.norm_q, s.norm_k = dev(get(p + ".attn.norm_q.weight"), float32), dev(get(p + ".attn.norm_k.weight"), float32)
            if s.out_w.shape[1] != D + s.mlp_w.shape[0]:
                raise ValueError(f"FluxTransformer: {p}.proj_out takes {s.out_w.shape[1]} columns, expected {D} + {s.mlp_w.shape[0]}")
            self.single.append(s)
        self._rope: "dict[bytes, tuple[GPUArray, GPUArray]]" = {}
        self._ctx: "GPUArray | None" = None
        self._pooled: "GPUArray | None" = None
        self._ctx_shape = (0, 0)
        self.encoder_projections = 0

    # ------------------------------------------------------------------ loading
    @classmethod
    def from_safetensors(cls, path, dtype: "str | DataType" = "float32", config: "FluxConfig | None" = None) -> "FluxTransformer":
        """A file, or a directory whose *.safetensors files (a sharded checkpoint) are all read.  The config is read off the
        tensors (_detect_config) unless given."""
        from pygpukit_amd.llm.safetensors import load_safetensors

        path = Path(path)
        if path.is_dir():
            files = sorted(path.glob("*.safetensors")) or sorted(path.glob("**/*.safetensors"))
            if not files:
                raise FileNotFoundError(f"No safetensors files found in {path}")
        elif path.exists():
            files = [path]
        else:
            raise FileNotFoundError(f"No safetensors file at {path}")
        weights = {}
        for f in files:
            st = load_safetensors(str(f))
            for name in st.tensor_names:
                weights[name] = st.tensor_as_f32(name)
        return cls(config or cls._detect_config(weights), weights, dtype=dtype)

    @staticmethod
    def _detect_config(weights: dict) -> FluxConfig:
        """Blocks counted, sizes read off the tensors (the reference reads the hidden size and counts the blocks, and takes
        FLUX.1's defaults for the rest): head_dim from attn.norm_q, the RoPE axes (16, 56, 56) at head_dim 128 and
        (d / 4, 3 d / 8, 3 d / 8) otherwise."""
        def count(prefix):
            return 1 + max((int(k.split(".")[1]) for k in weights if k.startswith(prefix)), default=-1)

        default = FluxConfig()
        hidden = int(weights["x_embedder.weight"].shape[0]) if "x_embedder.weight" in weights else default.hidden_size
        cfg = FluxConfig(hidden_size=hidden, num_layers=count("transformer_blocks."), num_single_layers=count("single_transformer_blocks."),
                         guidance_embeds="time_text_embed.guidance_embedder.linear_1.weight" in weights)
        if "x_embedder.weight" in weights:
            cfg.in_channels = int(weights["x_embedder.weight"].shape[1])
        if "proj_out.weight" in weights and int(weights["proj_out.weight"].shape[0]) != cfg.in_channels:
            cfg.out_channels = int(weights["proj_out.weight"].shape[0])
        if "context_embedder.weight" in weights:
            cfg.joint_attention_dim = int(weights["context_embedder.weight"].shape[1])
        if "time_text_embed.text_embedder.linear_1.weight" in weights:
            cfg.pooled_projection_dim = int(weights["time_text_embed.text_embedder.linear_1.weight"].shape[1])
        norm_q = next((v for k, v in weights.items() if k.endswith(".attn.norm_q.weight")), None)
        if norm_q is not None:
            hd = int(norm_q.shape[0])
            cfg.attention_head_dim, cfg.num_attention_heads = hd, hidden // hd
            if hd != 128:
                cfg.axes_dims_rope = (hd // 4, 3 * hd // 8, 3 * hd // 8)
        return cfg

    # ------------------------------------------------------------------ prompt-only work
    def set_encoder_states(self, encoder_hidden_states: GPUArray, pooled_projections: GPUArray) -> None:
        """context_embedder on the text tokens and the pooled text_embedder MLP (Linear, SiLU, Linear), once per prompt."""
        e, c = encoder_hidden_states, self.config
        if e.ndim != 3 or e.shape[2] != c.joint_attention_dim or e.shape[0] < 1 or e.shape[1] < 1:
            raise ValueError(f"FluxTransformer: encoder_hidden_states must be [B, tokens, {c.joint_attention_dim}], got {e.shape}")
        B, T, _ = e.shape
        if pooled_projections.shape != (B, c.pooled_projection_dim):
            raise ValueError(f"FluxTransformer: pooled_projections must be [{B}, {c.pooled_projection_dim}], got {pooled_projections.shape}")
        self._ctx = matmul_nt(e.astype(self.dtype)._view(0, (B * T, e.shape[2])), self.ctx_w, self.ctx_b)
        h = matmul_nt(pooled_projections.astype(float32), self.p1_w, self.p1_b)
        self._pooled = matmul_nt(silu(h, out=h), self.p2_w, self.p2_b)
        self._ctx_shape = (B, T)
        self.encoder_projections += 1

    # ------------------------------------------------------------------ pieces
    def _rope_tables(self, img_ids: np.ndarray, txt_ids: np.ndarray) -> "tuple[GPUArray, GPUArray]":
        img_ids, txt_ids = np.ascontiguousarray(img_ids), np.ascontiguousarray(txt_ids)
        key = str((img_ids.shape, img_ids.dtype.str, txt_ids.shape, txt_ids.dtype.str)).encode() + img_ids.tobytes() + txt_ids.tobytes()
        if key not in self._rope:
            cos, sin = get_rope_frequencies(img_ids, txt_ids, axes_dim=self.config.axes_dims_rope)
            self._rope[key] = (from_numpy(cos), from_numpy(sin))
        return self._rope[key]

    @staticmethod
    def _vector(v, B: int, what: str) -> np.ndarray:
        if isinstance(v, GPUArray):
            v = v.astype(float32).to_numpy()
        v = np.asarray(v, dtype=np.float32).reshape(-1)
        if v.size == 1:
            v = np.repeat(v, B)
        if v.size != B:
            raise ValueError(f"FluxTransformer: {v.size} {what} values for a batch of {B}")
        return v

    def _mlp(self, x: np.ndarray, w1, b1, w2, b2) -> GPUArray:
        h = matmul_nt(from_numpy(x), w1, b1)
        return matmul_nt(silu(h, out=h), w2, b2)

    def _modulations(self, timestep, guidance, B: int) -> GPUArray:
        """-> the projection of silu(temb) through the packed matrix, [B, rows] in the model dtype."""
        temb = self._mlp(timestep_embedding(self._vector(timestep, B, "timestep"), TIME_EMBED_DIM), self.t1_w, self.t1_b, self.t2_w, self.t2_b)
        add(temb, self._pooled, out=temb)
        if self.config.guidance_embeds and guidance is not None:
            g = self._mlp(timestep_embedding(self._vector(guidance, B, "guidance") * 1000, TIME_EMBED_DIM), self.g1_w, self.g1_b, self.g2_w,
                          self.g2_b)
            add(temb, g, out=temb)
        return matmul_nt(silu(temb, out=temb).astype(self.dtype), self.mod_w, self.mod_b)

    # ------------------------------------------------------------------ forward
    def forward(self, hidden_states: GPUArray, encoder_hidden_states: "GPUArray | None" = None, pooled_projections: "GPUArray | None" = None,
                timestep=None, img_ids=None, txt_ids=None, guidance=None) -> GPUArray:
        """timestep (fed to the sinusoid as given) and guidance: one value for the batch or one per element.  With
        encoder_hidden_states and pooled_projections the prompt-only work runs first (the reference's semantics); without, the
        states of the last set_encoder_states call are reused.  img_ids / txt_ids: [n, 3] or [B, n, 3], of which batch element
        0 serves the whole batch (the reference's behaviour); None: a square image grid and running text indices."""
        c = self.config
        if hidden_states.ndim != 3 or hidden_states.shape[2] != c.in_channels:
            raise ValueError(f"FluxTransformer: hidden_states must be [B, tokens, {c.in_channels}], got {hidden_states.shape}")
        if timestep is None:
            raise ValueError("FluxTransformer: timestep is required")
        if (encoder_hidden_states is None) != (pooled_projections is None):
            raise ValueError("FluxTransformer: encoder_hidden_states and pooled_projections go together")
        if encoder_hidden_states is not None:
            self.set_encoder_states(encoder_hidden_states, pooled_projections)
        if self._ctx is None:
            raise RuntimeError("FluxTransformer: no encoder states - pass encoder_hidden_states and pooled_projections or call "
                               "set_encoder_states first")
        B, I, _ = hidden_states.shape
        if B != self._ctx_shape[0]:
            raise ValueError(f"FluxTransformer: hidden_states batch {B} != encoder states batch {self._ctx_shape[0]}")
        T = self._ctx_shape[1]
        if img_ids is None:
            side = int(np.sqrt(I))
            if side * side != I:
                raise ValueError(f"FluxTransformer: {I} image tokens are no square grid - pass img_ids")
            img_ids = prepare_image_ids(B, side, side)
        if txt_ids is None:
            txt_ids = prepare_text_ids(B, T)
        img_ids, txt_ids = (np.asarray(a)[0] if np.asarray(a).ndim == 3 else np.asarray(a) for a in (img_ids, txt_ids))
        if img_ids.shape != (I, 3) or txt_ids.shape != (T, 3):
            raise ValueError(f"FluxTransformer: ids must be [{I}, 3] and [{T}, 3], got {img_ids.shape} and {txt_ids.shape}")
        cos, sin = self._rope_tables(img_ids, txt_ids)
        proj = self._modulations(timestep, guidance, B)
        hidden = hidden_states.astype(self.dtype)
        out = GPUArray((B, I, self.out_channels), self.dtype)
        for b in range(B):
            self._element(hidden._view(b * I * c.in_channels, (I, c.in_channels)), self._ctx._view(b * T * self.hidden_size, (T, self.hidden_size)),
                          proj, b, cos, sin, out._view(b * I * self.out_channels, (I, self.out_channels)))
        return out

    __call__ = forward

    def _element(self, hidden: GPUArray, ctx: GPUArray, proj: GPUArray, b: int, cos: GPUArray, sin: GPUArray, out: GPUArray) -> None:
        D, H, hd, dt = self.hidden_size, self.num_heads, self.head_dim, self.dtype
        I, T = hidden.shape[0], ctx.shape[0]
        S = T + I
        L, Ls = len(self.double), len(self.single)
        base = b * self.layout["rows"]

        def mod(offset: int, k: int) -> Modulation:
            return Modulation(vector=proj, vector_offset=base + offset + k * D, stride=0)

        x = GPUArray((S, D), dt)            # the residual stream, text rows first
        h = GPUArray((S, D), dt)            # the modulated norm the next sub-layer reads
        qkv = GPUArray((S, 3 * D), dt)
        attn = GPUArray((S, D), dt)

        def rows(a: GPUArray, lo: int, hi: int, as3: bool = False) -> GPUArray:
            width = a.shape[-1]
            return a._view(lo * width, (1, hi - lo, width) if as3 else (hi - lo, width))

        streams = ((0, T), (T, S))          # text, image

        def next_input(i: int, stream: int):
            """(scale, shift) of the modulated norm that follows double block i - 1 (i counts double blocks, then single blocks);
            None where nothing reads the rows again."""
            if i < L:
                off = self.layout["double"][i][1 - stream]      # stream 0 = text = norm1_context
                return mod(off, 1), mod(off, 0)
            if i - L < Ls:
                off = self.layout["single"][i - L]
                return mod(off, 1), mod(off, 0)
            return (mod(self.layout["out"], 0), mod(self.layout["out"], 1)) if stream == 1 else None

        def attention(out_buf: GPUArray, out_row: int) -> None:
            sdpa_noncausal_strided(qkv, qkv._view(D, (qkv.size - D,)), qkv._view(2 * D, (qkv.size - 2 * D,)), out_buf, H, H, S, S, hd,
                                   (hd, 3 * D), (hd, 3 * D), (hd, out_row), self.attn_scale)

        matmul_nt(hidden, self.x_w, self.x_b, out=rows(x, T, S))
        copy_to(ctx, rows(x, 0, T))
        for s, (lo, hi) in enumerate(streams):
            nxt = next_input(0, s)
            if nxt is not None:
                gated_residual_adaln(rows(x, lo, hi, True), None, None, *nxt, EPS, out=rows(h, lo, hi, True))

        for i, blk in enumerate(self.double):
            off_img, off_txt = self.layout["double"][i]
            matmul_nt(rows(h, 0, T), blk.add_qkv_w, blk.add_qkv_b, out=rows(qkv, 0, T))
            matmul_nt(rows(h, T, S), blk.qkv_w, blk.qkv_b, out=rows(qkv, T, S))
            flux_qk_norm_rope(qkv, qkv._view(D, (qkv.size - D,)), cos, sin, blk.norm_added_q, blk.norm_added_k, batch=1, seq=S, heads=H,
                              head_dim=hd, row_stride=3 * D, split=T, wq_b=blk.norm_q, wk_b=blk.norm_k, eps=EPS)
            attention(attn, D)
            for s, (lo, hi) in enumerate(streams):
                off = off_txt if s == 0 else off_img
                w_o, b_o = (blk.add_out_w, blk.add_out_b) if s == 0 else (blk.out_w, blk.out_b)
                f1w, f1b, f2w, f2b = (blk.ffc1_w, blk.ffc1_b, blk.ffc2_w, blk.ffc2_b) if s == 0 else (blk.ff1_w, blk.ff1_b, blk.ff2_w, blk.ff2_b)
                xs = rows(x, lo, hi, True)
                a = matmul_nt(rows(attn, lo, hi), w_o, b_o)
                a3 = a._view(0, (1, hi - lo, D))
                gated_residual_adaln(a3, xs, mod(off, 2), mod(off, 4), mod(off, 3), EPS, sum_out=xs, out=a3)
                f = matmul_nt(linear_bias_gelu(a, f1w, f1b), f2w, f2b)
                f3 = f._view(0, (1, hi - lo, D))
                nxt = next_input(i + 1, s)
                if nxt is None:
                    gated_residual(xs, mod(off, 5), f3, out=xs)
                else:
                    gated_residual_adaln(f3, xs, mod(off, 5), *nxt, EPS, sum_out=xs, out=rows(h, lo, hi, True))

        if Ls:
            mlp_dim = self.single[0].mlp_w.shape[0]
            mlp = GPUArray((S, mlp_dim), dt)
            cat = GPUArray((S, D + mlp_dim), dt)
        for j, blk in enumerate(self.single):
            off = self.layout["single"][j]
            matmul_nt(h, blk.qkv_w, blk.qkv_b, out=qkv)
            matmul_nt(h, blk.mlp_w, blk.mlp_b, out=mlp)
            flux_qk_norm_rope(qkv, qkv._view(D, (qkv.size - D,)), cos, sin, blk.norm_q, blk.norm_k, batch=1, seq=S, heads=H, head_dim=hd,
                              row_stride=3 * D, eps=EPS)
            attention(cat, D + mlp_dim)
            flux_gelu_pack(mlp, cat, column=D)
            o = matmul_nt(cat, blk.out_w, blk.out_b)
            if j + 1 < Ls:
                gated_residual_adaln(o._view(0, (1, S, D)), x._view(0, (1, S, D)), mod(off, 2), *next_input(L + j + 1, 1), EPS,
                                     sum_out=x._view(0, (1, S, D)), out=h._view(0, (1, S, D)))
            else:                           # after the last block only the image rows are read again, by norm_out
                xi = rows(x, T, S, True)
                gated_residual_adaln(rows(o, T, S, True), xi, mod(off, 2), *next_input(L + Ls, 1), EPS, sum_out=xi, out=rows(h, T, S, True))
        matmul_nt(rows(h, T, S), self.proj_w, self.proj_b, out=out)


__all__ = ["FluxConfig", "FluxTransformer", "flux_plan", "modulation_layout", "modulation_names", "pack_qkv"]
