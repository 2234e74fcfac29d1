"""PixArt-Sigma transformer (reference: src/pygpukit/diffusion/models/dit/model.py).  The computation is the reference's, quirks
included (INTEGRATION.md "Diffusion transformer"); the reference runs every norm, modulation, softmax and residual on the host in
NumPy and only the matmuls on the device - here everything stays on the device:

  * per block FIVE GEMMs (fused q|k|v, attention out, cross-attention q, cross-attention out, two FFN GEMMs counted with their
    fused bias), two attentions reading the projections in place (sdpa_noncausal_strided), and THREE launches of the fused row
    kernel (diffusion.ops.gated_residual_adaln): the gated self-attention residual; the cross-attention residual with the FFN's
    modulated norm; the gated FFN residual with the NEXT block's modulated norm (the final layer's after the last block);
  * the six modulation vectors of a block are read in place from its scale_shift_table [6, D] and the adaln_single output
    [B, 6, D] (float32, like the position table and the whole conditioning path): no sum, no broadcast is ever materialised;
  * set_encoder_states runs the caption projection and every block's cross-attention K | V projection once per prompt;
    forward(latent, timestep) reuses them on every denoising step;
  * 16-bit dtypes with a head_dim that the MFMA flash kernel does not take (PixArt: 72) can pack the attention weights at load
    time so that each head occupies 64 or 128 columns (zero rows in the q / k / v weights and biases, zero columns in the out
    projections); with scale = 1 / sqrt(real head_dim) passed explicitly the result is exact - the zero tails add nothing to
    Q K^T or to P V.  `pad_heads` = "auto" | True | False, see dit_plan."""

from __future__ import annotations

import os
from pathlib import Path

import numpy as np

from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import DataType, as_dtype, float32
from pygpukit_amd.core.factory import from_numpy
from pygpukit_amd.diffusion.config import PixArtSpec
from pygpukit_amd.diffusion.models.dit.embeddings import get_2d_sincos_pos_embed, sinusoidal_embedding
from pygpukit_amd.diffusion.ops.adaln import Modulation, gated_residual, gated_residual_adaln
from pygpukit_amd.diffusion.ops.patch import patchify, unpatchify
from pygpukit_amd.ops.elementwise import add
from pygpukit_amd.ops.matmul import linear_bias_gelu, matmul_nt
from pygpukit_amd.ops.nn.activation import silu
from pygpukit_amd.ops.nn.attention import sdpa_noncausal_strided
from pygpukit_amd.ops.nn.fused import glu_packed

LN_EPS = 1e-6            # the reference's models/dit layer_norm
TIME_EMBED_DIM = 256     # sinusoidal input width of adaln_single.emb.timestep_embedder
# pad_heads="auto": padding to the flash kernel's head width against the one-workgroup-per-query-row fallback, decided by
# tools/dit_bench.py section (b) at PixArt-Sigma's shape (profiles/r15_dit_bench.log): 16 heads of 72, 4096 tokens, bf16 -
# padded flash 176 us against 77 ms for the fallback (439x), cross-attention on 300 keys 28 us against 4.8 ms (170x)
AUTO_PAD_HEADS = True


def dit_plan(spec, dtype, pad_heads="auto") -> dict:
    """What the model will run for `spec` in `dtype`: {"head_dim", "head_width" (columns a head occupies in the projections),
    "padded", "attention": "flash" | "fallback"}.  Heads are padded only for bfloat16 / float16 with a head_dim other than 64 /
    128 and at most 128: pad_heads=True always, "auto" as AUTO_PAD_HEADS says, False never.  float32 always runs the fallback
    kernel, so it is never padded.  PYGPUKIT_FLASH_ATTENTION=0 turns the flash kernel off in the library; the plan reports it."""
    if pad_heads not in ("auto", True, False):
        raise ValueError(f"pad_heads must be 'auto', True or False, got {pad_heads!r}")
    dt = as_dtype(dtype)
    hd = spec.get_head_dim()
    flash_on = os.environ.get("PYGPUKIT_FLASH_ATTENTION") not in ("0", "false")
    width = hd
    if dt != float32 and hd not in (64, 128) and hd <= 128 and (AUTO_PAD_HEADS if pad_heads == "auto" else pad_heads):
        width = 64 if hd < 64 else 128
    flash = dt != float32 and width in (64, 128) and flash_on
    return {"head_dim": hd, "head_width": width, "padded": width != hd, "attention": "flash" if flash else "fallback"}


def pack_head_rows(w: np.ndarray, heads: int, head_dim: int, width: int) -> np.ndarray:
    """[heads * head_dim, ...] -> [heads * width, ...]: head h's rows at h * width, zero rows after them (q / k / v weights, biases)."""
    if width == head_dim:
        return np.ascontiguousarray(w)
    out = np.zeros((heads * width,) + w.shape[1:], w.dtype)
    out.reshape((heads, width) + w.shape[1:])[:, :head_dim] = w.reshape((heads, head_dim) + w.shape[1:])
    return out


def pack_head_columns(w: np.ndarray, heads: int, head_dim: int, width: int) -> np.ndarray:
    """[out, heads * head_dim] -> [out, heads * width] with zero columns (the attention out projections)."""
    return np.ascontiguousarray(pack_head_rows(np.ascontiguousarray(w.T), heads, head_dim, width).T)


def _host(a) -> np.ndarray:
    if isinstance(a, GPUArray):
        a = a.astype(float32).to_numpy()
    return np.ascontiguousarray(a, dtype=np.float32)


class _Block:
    __slots__ = ("table", "qkv_w", "qkv_b", "out_w", "out_b", "q2_w", "q2_b", "kv2_w", "kv2_b", "out2_w", "out2_b", "ff1_w", "ff1_b",
                 "ff2_w", "ff2_b", "geglu", "ff_dim")


class PixArtTransformer:
    """forward(latent [B, C, H, W], timestep, encoder_hidden_states [B, M, text_dim]) -> [B, out_channels, H, W] in `dtype`."""

    def __init__(self, spec: PixArtSpec, weights: dict, dtype: "str | DataType" = "float32", pad_heads="auto"):
        self.spec = spec
        self.dtype = as_dtype(dtype)
        self.hidden_size = D = spec.hidden_size
        self.num_layers = spec.num_layers
        self.num_heads = H = spec.num_heads
        self.head_dim = hd = spec.get_head_dim()
        self.patch_size = spec.patch_size
        if H * hd != D:
            raise ValueError(f"PixArtTransformer: hidden_size {D} is not {H} heads of {hd}")
        self.plan = dit_plan(spec, self.dtype, pad_heads)
        self.head_width = width = self.plan["head_width"]
        self.attn_scale = 1.0 / float(np.sqrt(hd))

        def get(name):
            if name not in weights:
                raise KeyError(f"PixArtTransformer: missing tensor {name}")
            return _host(weights[name])

        def dev(a, dt=None):
            return from_numpy(np.ascontiguousarray(a, dtype=np.float32)).astype(dt or self.dtype)

        # float32 whatever the dtype: patch embedding (K = C p p, a tiny GEMM), the conditioning path, the modulation tables
        self.patch_w = dev(get("pos_embed.proj.weight").reshape(D, -1), float32)
        self.patch_b = dev(get("pos_embed.proj.bias"), float32)
        te = "adaln_single.emb.timestep_embedder."
        self.t1_w, self.t1_b = dev(get(te + "linear_1.weight"), float32), dev(get(te + "linear_1.bias"), float32)
        self.t2_w, self.t2_b = dev(get(te + "linear_2.weight"), float32), dev(get(te + "linear_2.bias"), float32)
        self.ada_w, self.ada_b = dev(get("adaln_single.linear.weight"), float32), dev(get("adaln_single.linear.bias"), float32)
        self.final_table = dev(get("scale_shift_table"), float32)                                   # [2, D]: shift, scale
        if self.t1_w.shape[1] != TIME_EMBED_DIM:
            raise ValueError(f"PixArtTransformer: timestep_embedder.linear_1 must take {TIME_EMBED_DIM} inputs, got {self.t1_w.shape[1]}")
        self.cap1_w, self.cap1_b = dev(get("caption_projection.linear_1.weight")), dev(get("caption_projection.linear_1.bias"))
        self.cap2_w, self.cap2_b = dev(get("caption_projection.linear_2.weight")), dev(get("caption_projection.linear_2.bias"))
        self.proj_w, self.proj_b = dev(get("proj_out.weight")), dev(get("proj_out.bias"))
        if self.proj_w.shape[0] != spec.patch_size ** 2 * spec.out_channels:
            raise ValueError(f"PixArtTransformer: proj_out has {self.proj_w.shape[0]} rows, expected p*p*out_channels")

        def rows(name):
            return pack_head_rows(get(name), H, hd, width)

        self.blocks = []
        for i in range(self.num_layers):
            p, b = f"transformer_blocks.{i}.", _Block()
            b.table = dev(get(p + "scale_shift_table"), float32)                                    # [6, D]
            b.qkv_w = dev(np.concatenate([rows(p + f"attn1.to_{n}.weight") for n in "qkv"]))        # [3 H width, D]
            b.qkv_b = dev(np.concatenate([rows(p + f"attn1.to_{n}.bias") for n in "qkv"]))
            b.out_w = dev(pack_head_columns(get(p + "attn1.to_out.0.weight"), H, hd, width))        # [D, H width]
            b.out_b = dev(get(p + "attn1.to_out.0.bias"))
            b.q2_w, b.q2_b = dev(rows(p + "attn2.to_q.weight")), dev(rows(p + "attn2.to_q.bias"))
            b.kv2_w = dev(np.concatenate([rows(p + f"attn2.to_{n}.weight") for n in "kv"]))         # [2 H width, D]
            b.kv2_b = dev(np.concatenate([rows(p + f"attn2.to_{n}.bias") for n in "kv"]))
            b.out2_w = dev(pack_head_columns(get(p + "attn2.to_out.0.weight"), H, hd, width))
            b.out2_b = dev(get(p + "attn2.to_out.0.bias"))
            w1, w2 = get(p + "ff.net.0.proj.weight"), get(p + "ff.net.2.weight")
            b.ff_dim = w2.shape[1]
            b.geglu = w1.shape[0] == 2 * b.ff_dim                     # the reference's rule: GEGLU when the halves fit ff.net.2
            if not b.geglu and w1.shape[0] != b.ff_dim:
                raise ValueError(f"PixArtTransformer: {p}ff.net.0.proj has {w1.shape[0]} rows for {b.ff_dim} columns of ff.net.2")
            b.ff1_w, b.ff1_b = dev(w1), dev(get(p + "ff.net.0.proj.bias"))
            b.ff2_w, b.ff2_b = dev(w2), dev(get(p + "ff.net.2.bias"))
            self.blocks.append(b)
        self._pos: dict[tuple[int, int, int], GPUArray] = {}
        self._kv: "list[GPUArray] | None" = None
        self._ctx_shape = (0, 0)
        self.encoder_projections = 0        # times set_encoder_states ran (a forward with two arguments must not raise it)

    # ------------------------------------------------------------------ loading
    @classmethod
    def from_safetensors(cls, path, dtype: "str | DataType" = "float32", pad_heads="auto") -> "PixArtTransformer":
        """A model directory (diffusion_pytorch_model.safetensors, else its first *.safetensors) or a file.  The spec is read off
        the tensors as the reference does: hidden size from pos_embed.proj.bias, blocks counted, head_dim 72."""
        from pygpukit_amd.llm.safetensors import load_safetensors

        path = Path(path)
        if path.is_dir():
            model_path = path / "diffusion_pytorch_model.safetensors"
            if not model_path.exists():
                found = sorted(path.glob("*.safetensors"))
                if not found:
                    raise FileNotFoundError(f"No safetensors found in {path}")
                model_path = found[0]
        else:
            model_path = path
        st = load_safetensors(str(model_path))
        weights = {name: st.tensor_as_f32(name) for name in st.tensor_names}
        hidden = int(weights["pos_embed.proj.bias"].shape[0])
        blocks = sum(1 for k in weights if k.startswith("transformer_blocks.") and k.endswith(".attn1.to_q.weight"))
        text_dim = int(weights["caption_projection.linear_1.weight"].shape[1])
        pw = weights["pos_embed.proj.weight"]
        out_channels = int(weights["proj_out.weight"].shape[0]) // (int(pw.shape[2]) * int(pw.shape[3]))
        spec = PixArtSpec(name="pixart_sigma", hidden_size=hidden, num_layers=blocks, num_heads=hidden // 72,
                          conditioning_type="cross_attn", text_encoder_dim=text_dim, pos_embed_type="sinusoidal",
                          patch_size=int(pw.shape[2]), in_channels=int(pw.shape[1]), out_channels=out_channels,
                          cross_attention_dim=text_dim)
        return cls(spec, weights, dtype=dtype, pad_heads=pad_heads)

    # ------------------------------------------------------------------ prompt-only work
    def set_encoder_states(self, encoder_hidden_states: GPUArray) -> None:
        """Caption projection (Linear, SiLU, Linear) and every block's cross-attention K | V (one GEMM per block) for this prompt;
        forward(latent, timestep) then reuses them."""
        e = encoder_hidden_states
        if e.ndim != 3 or e.shape[2] != self.cap1_w.shape[1]:
            raise ValueError(f"PixArtTransformer: encoder_hidden_states must be [B, tokens, {self.cap1_w.shape[1]}], got {e.shape}")
        B, M, _ = e.shape
        if B < 1 or M < 1:
            raise ValueError(f"PixArtTransformer: empty encoder_hidden_states {e.shape}")
        h = matmul_nt(e.astype(self.dtype)._view(0, (B * M, e.shape[2])), self.cap1_w, self.cap1_b)
        ctx = matmul_nt(silu(h, out=h), self.cap2_w, self.cap2_b)
        self._kv = [matmul_nt(ctx, b.kv2_w, b.kv2_b) for b in self.blocks]
        self._ctx_shape = (B, M)
        self.encoder_projections += 1

    # ------------------------------------------------------------------ pieces
    def _position_table(self, B: int, hp: int, wp: int) -> GPUArray:
        key = (B, hp, wp)
        if key not in self._pos:
            self._pos[key] = from_numpy(np.tile(get_2d_sincos_pos_embed(self.hidden_size, (hp, wp)), (B, 1)))
        return self._pos[key]

    def _conditioning(self, timestep, B: int) -> "tuple[GPUArray, GPUArray]":
        """-> t_emb [B, D], adaln_single output [B, 6 D], both float32."""
        if isinstance(timestep, GPUArray):
            timestep = timestep.astype(float32).to_numpy()
        t = np.asarray(timestep, dtype=np.float32).reshape(-1)
        if t.size == 1:
            t = np.repeat(t, B)
        if t.size != B:
            raise ValueError(f"PixArtTransformer: {t.size} timesteps for a batch of {B}")
        h = matmul_nt(from_numpy(sinusoidal_embedding(t, TIME_EMBED_DIM)), self.t1_w, self.t1_b)
        t_emb = matmul_nt(silu(h, out=h), self.t2_w, self.t2_b)
        return t_emb, matmul_nt(silu(t_emb), self.ada_w, self.ada_b)

    def _attention(self, q: GPUArray, q_off: int, q_row: int, kv: GPUArray, k_off: int, kv_row: int, B: int, n_q: int, n_kv: int) -> GPUArray:
        """Per batch element, straight off the projections: q rows of q_row elements starting at q_off, K at k_off and V one
        projection width after it in rows of kv_row elements.  -> [B * n_q, H * width]."""
        H, width = self.num_heads, self.head_width
        dp = H * width
        out = GPUArray((B * n_q, dp), self.dtype)
        for b in range(B):
            qb, kb = b * n_q * q_row + q_off, b * n_kv * kv_row + k_off
            sdpa_noncausal_strided(q._view(qb, (q.size - qb,)), kv._view(kb, (kv.size - kb,)), kv._view(kb + dp, (kv.size - kb - dp,)),
                                   out._view(b * n_q * dp, (n_q, dp)), H, H, n_q, n_kv, width, (width, q_row), (width, kv_row),
                                   (width, dp), self.attn_scale)
        return out

    def _ffn(self, blk: _Block, h: GPUArray) -> GPUArray:
        if blk.geglu:
            return matmul_nt(glu_packed(matmul_nt(h, blk.ff1_w, blk.ff1_b), blk.ff_dim, activation="gelu"), blk.ff2_w, blk.ff2_b)
        return matmul_nt(linear_bias_gelu(h, blk.ff1_w, blk.ff1_b), blk.ff2_w, blk.ff2_b)

    # ------------------------------------------------------------------ forward
    def forward(self, latent: GPUArray, timestep, encoder_hidden_states: "GPUArray | None" = None, pooled_projections=None,
                guidance=None) -> GPUArray:
        """timestep: a scalar for the whole batch or one value per element.  With encoder_hidden_states the prompt-only work runs
        first (the reference's semantics); without, the states of the last set_encoder_states call are reused."""
        if latent.ndim != 4 or latent.shape[1] != self.spec.in_channels:
            raise ValueError(f"PixArtTransformer: latent must be [B, {self.spec.in_channels}, H, W], got {latent.shape}")
        if encoder_hidden_states is not None:
            self.set_encoder_states(encoder_hidden_states)
        if self._kv is None:
            raise RuntimeError("PixArtTransformer: no encoder states - pass encoder_hidden_states or call set_encoder_states first")
        B, _, Hh, Ww = latent.shape
        if B != self._ctx_shape[0]:
            raise ValueError(f"PixArtTransformer: latent batch {B} != encoder states batch {self._ctx_shape[0]}")
        p, D, M = self.patch_size, self.hidden_size, self._ctx_shape[1]
        if Hh % p or Ww % p:
            raise ValueError(f"PixArtTransformer: H={Hh} and W={Ww} must be multiples of the patch size {p}")
        hp, wp = Hh // p, Ww // p
        N = hp * wp
        dp = self.num_heads * self.head_width

        x32 = matmul_nt(patchify(latent.astype(float32), p), self.patch_w, self.patch_b)            # [B N, D]
        x = add(x32, self._position_table(B, hp, wp), out=x32).astype(self.dtype)
        t_emb, cond = self._conditioning(timestep, B)

        def mod(i: int, k: int) -> Modulation:
            return Modulation(self.blocks[i].table, cond, table_offset=k * D, vector_offset=k * D, stride=6 * D)

        def input_modulation(i: int):
            """(scale, shift) of block i's first modulated norm; of the final layer for i == num_layers."""
            if i < self.num_layers:
                return mod(i, 1), mod(i, 0)
            return Modulation(self.final_table, table_offset=D), Modulation(self.final_table, t_emb)

        def rows3(a: GPUArray) -> GPUArray:
            return a._view(0, (B, N, D))

        x3 = rows3(x)
        h = gated_residual_adaln(x3, None, None, *input_modulation(0), LN_EPS)[1]
        for i, blk in enumerate(self.blocks):
            qkv = matmul_nt(h._view(0, (B * N, D)), blk.qkv_w, blk.qkv_b)                           # [B N, 3 dp]: q | k | v per row
            a = matmul_nt(self._attention(qkv, 0, 3 * dp, qkv, dp, 3 * dp, B, N, N), blk.out_w, blk.out_b)
            gated_residual(x3, mod(i, 2), rows3(a), out=x3)
            q = matmul_nt(x, blk.q2_w, blk.q2_b)
            c = matmul_nt(self._attention(q, 0, dp, self._kv[i], 0, 2 * dp, B, N, M), blk.out2_w, blk.out2_b)
            _, h = gated_residual_adaln(rows3(c), x3, None, mod(i, 4), mod(i, 3), LN_EPS, sum_out=x3, out=rows3(c))
            f = self._ffn(blk, h._view(0, (B * N, D)))
            _, h = gated_residual_adaln(rows3(f), x3, mod(i, 5), *input_modulation(i + 1), LN_EPS, sum_out=x3, out=rows3(f))
        y = matmul_nt(h._view(0, (B * N, D)), self.proj_w, self.proj_b)
        return unpatchify(y, B, self.spec.out_channels, Hh, Ww, p)

    __call__ = forward


__all__ = ["PixArtTransformer", "dit_plan", "pack_head_rows", "pack_head_columns"]
