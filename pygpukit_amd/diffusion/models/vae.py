"""VAE decoder (reference: src/pygpukit/diffusion/models/vae.py, whose decoder is a placeholder: conv_in, then scipy's zoom).
Here decode runs the AutoencoderKL decoder that the SD / SDXL / SD3 / Flux checkpoints hold (diffusers tensor names), on the
device from the latent to the image:

    x = latent / scaling_factor + shift_factor
    post_quant_conv (1x1, if present) -> decoder.conv_in -> mid_block (resnet, attention, resnet)
    -> up_blocks over reversed(block_out_channels) (layers_per_block + 1 resnets, nearest 2x + 3x3 on all but the last)
    -> conv_norm_out + SiLU -> conv_out -> clamp to [-1, 1]
    resnet: GN -> SiLU -> conv3x3 -> GN -> SiLU -> conv3x3 + shortcut(x); the shortcut is a 1x1 conv when the channels change

Device residency.  Between conv_in and conv_out every activation is channels-last [B, H, W, C]: conv_in reads NCHW and writes
channels-last, conv_out does the reverse, so no transpose is ever launched.  Weights are packed once at load.  A resnet is 4
launches (two group_norm_silu, two conv2d - the residual add rides in the second convolution's epilogue), 5 with a shortcut
convolution; an upsampler is ONE conv2d (the nearest 2x is an index computation of its slab fill).  vae_plan counts them.

Mid-block attention: ONE head of dim C (512), which the MFMA flash kernel does not take.  The attention rows [H W, C] are the
channels-last activation itself.  Two paths, chosen per (tokens, dtype) by vae_plan:
  * "sdpa":   one fused q|k|v GEMM, sdpa_noncausal on the fallback kernel (keys <= 15360), out projection;
  * "matmul": q and k GEMMs, then per image V^T = W_v X^T as a GEMM (so no transpose), scores = q k^T (T x T elements per
              image), softmax, P (V^T)^T, out projection.
1 / sqrt(C) is folded into to_q and b_v into to_out's bias (b' = W_out b_v + b_out: softmax rows sum to 1) in fp32 before the
weights are rounded.  Contract, layouts, weight names and the 16-bit error floors: INTEGRATION.md."""

from __future__ import annotations

from pathlib import Path

import numpy as np

from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import DataType, as_dtype, float32
from pygpukit_amd.core.factory import from_numpy
from pygpukit_amd.diffusion.config import SD3_VAE_SPEC, SDXL_VAE_SPEC, VAESpec
from pygpukit_amd.ops.conv import conv2d, conv2d_pack_weight, conv2d_plan
from pygpukit_amd.ops.elementwise import add, clamp, div
from pygpukit_amd.ops.matmul import matmul_nt
from pygpukit_amd.ops.nn.attention import sdpa_noncausal_strided
from pygpukit_amd.ops.nn.norm import group_norm, group_norm_plan, group_norm_silu
from pygpukit_amd.ops.reduction import softmax

SDPA_MAX_KEYS = 15360          # the fallback attention kernel keeps a row's scores in LDS
# attention="auto": the composition on the GEMM kernels above this many tokens, the fallback kernel (one workgroup per query
# row, 512-wide dot products on the vector ALU) at or below it.  Measured per dtype at 64, 256, 1024, 4096 and 16384 tokens, one
# image (tools/vae_bench.py section (d), profiles/r16_vae_bench.log).  float32: the fallback kernel wins at 64 and 256 tokens
# (0.5x and 0.7x the composition's time), loses at 1024 (2.1x) and 4096 (21x).  bfloat16: the composition is never slower -
# equal at 64 tokens (1.1x, inside the run's spread), 1.9x faster at 256, 16x at 1024, two orders of magnitude at 4096 - so the
# 16-bit dtypes always take it.  Above 15360 keys the fallback kernel does not run at all.
AUTO_SDPA_MAX_TOKENS = {"float32": 256, "float16": 0, "bfloat16": 0}


def _host(a) -> np.ndarray:
    if isinstance(a, GPUArray):
        a = a.astype(float32).to_numpy()
    return np.ascontiguousarray(a, dtype=np.float32)


def _up_blocks(spec) -> list:
    """[(c_in, c_out, has_upsampler)] per up block; every block has layers_per_block + 1 resnets, the first takes c_in."""
    rc = list(reversed(spec.block_out_channels))
    return [(rc[max(i - 1, 0)], ch, i < len(rc) - 1) for i, ch in enumerate(rc)]


def vae_plan(spec: VAESpec, dtype="float32", latent_hw=(64, 64), attention: str = "auto", post_quant: bool = True, batch: int = 1) -> dict:
    """What decode will run for `spec` in `dtype` on a [batch, latent_channels, *latent_hw] latent.  Host logic, no device:
      attention       "sdpa" | "matmul" (attention="auto": "matmul" in the 16-bit dtypes, and in float32 above 256 tokens, as
                      measured - AUTO_SDPA_MAX_TOKENS; forcing "sdpa" above 15360 tokens raises)
      tokens          H W of the mid block;  scores_bytes: the T x T score matrix of ONE image on the "matmul" path, else 0
      conv, group_norm  the plans of the decoder's largest 3x3 convolution and group normalisation
      launches        kernel launches of the whole decode, `resnet_launches` of them per resnet (4, or 5 with a shortcut)
      output_shape    [batch, out_channels, H 2^(stages-1), W 2^(stages-1)]"""
    if attention not in ("auto", "sdpa", "matmul"):
        raise ValueError(f"attention must be 'auto', 'sdpa' or 'matmul', got {attention!r}")
    dt = as_dtype(dtype)
    h, w = int(latent_hw[0]), int(latent_hw[1])
    if h < 1 or w < 1 or batch < 1:
        raise ValueError(f"vae_plan: empty latent {latent_hw} or batch {batch}")
    tokens = h * w
    path = attention
    if path == "auto":
        path = "sdpa" if tokens <= AUTO_SDPA_MAX_TOKENS.get(dt.name, 0) else "matmul"
    if path == "sdpa" and tokens > SDPA_MAX_KEYS:
        raise ValueError(f"vae_plan: the sdpa path takes at most {SDPA_MAX_KEYS} tokens, got {tokens}; use attention='matmul'")
    blocks = _up_blocks(spec)
    resnets = 2 * 4                                                   # mid block
    for c_in, c_out, _ in blocks:
        resnets += (5 if c_in != c_out else 4) + 4 * spec.layers_per_block
    n_up = sum(1 for b in blocks if b[2])
    pre = (1 if dt != float32 else 0) * 2 + 1 + (1 if spec.shift_factor != 0.0 else 0)   # casts around the fp32 div (+ add)
    attn = (4 + batch) if path == "sdpa" else (5 + 4 * batch)
    launches = pre + (1 if post_quant else 0) + 1 + resnets + attn + n_up + 1 + 1 + 1   # ... conv_in, norm_out, conv_out, clamp
    scale = 2 ** (len(spec.block_out_channels) - 1)
    c0 = spec.block_out_channels[0]
    return {"attention": path, "tokens": tokens, "scores_bytes": tokens * tokens * dt.itemsize if path == "matmul" else 0,
            "conv": conv2d_plan(c0, c0, h * scale, w * scale, 3, 1, 1, 1, dt),
            "group_norm": group_norm_plan(batch, c0, h * scale * w * scale, spec.norm_num_groups, dt, True),
            "resnet_launches": (4, 5), "launches": launches, "output_shape": (batch, spec.out_channels, h * scale, w * scale)}


class _Conv:
    __slots__ = ("w", "b", "packed", "pad")

    def __init__(self, w: np.ndarray, b: np.ndarray, dt: DataType):
        self.w = from_numpy(np.ascontiguousarray(w, dtype=np.float32)).astype(dt)
        self.b = from_numpy(np.ascontiguousarray(b, dtype=np.float32)).astype(dt)
        self.packed = conv2d_pack_weight(self.w) if dt != float32 else None
        self.pad = w.shape[2] // 2

    def __call__(self, x: GPUArray, *, cl_in=True, cl_out=True, upsample=1, add=None) -> GPUArray:
        return conv2d(x, self.w, self.b, 1, self.pad, channels_last=cl_in, channels_last_out=cl_out, upsample=upsample, add=add,
                      packed_weight=self.packed)


class _Resnet:
    __slots__ = ("n1", "c1", "n2", "c2", "shortcut")


class VAE:
    """decode(latent [B, latent_channels, H, W]) -> [B, 3, 8H, 8W] in `dtype`, clamped to [-1, 1]."""

    def __init__(self, spec: VAESpec, weights: "dict | None" = None, dtype: "str | DataType" = "float32", attention: str = "auto"):
        if attention not in ("auto", "sdpa", "matmul"):
            raise ValueError(f"attention must be 'auto', 'sdpa' or 'matmul', got {attention!r}")
        if not weights:
            raise ValueError("VAE: no weights - the decoder has no placeholder path (the reference upsamples with scipy there)")
        self.spec = spec
        self.dtype = dt = as_dtype(dtype)
        if dt.name not in ("float32", "float16", "bfloat16"):
            raise ValueError(f"VAE: dtype must be float32/float16/bfloat16, got {dt}")
        self.attention = attention
        self.groups, self.eps = spec.norm_num_groups, spec.norm_eps

        def get(name):
            for prefix in ("", "vae.", "first_stage_model."):
                if prefix + name in weights:
                    return _host(weights[prefix + name])
            raise KeyError(f"VAE: missing tensor {name}")

        def has(name):
            return any(p + name in weights for p in ("", "vae.", "first_stage_model."))

        def dev(a):
            return from_numpy(np.ascontiguousarray(a, dtype=np.float32)).astype(dt)

        def conv(name, c_out, c_in, k):
            w = get(name + ".weight")
            if w.shape != (c_out, c_in, k, k):
                raise ValueError(f"VAE: {name}.weight is {w.shape}, the spec needs {(c_out, c_in, k, k)}")
            return _Conv(w, get(name + ".bias"), dt)

        def norm(name, c):
            g = get(name + ".weight")
            if g.shape != (c,) or c % self.groups:
                raise ValueError(f"VAE: {name}.weight is {g.shape} for {c} channels in {self.groups} groups")
            return dev(g), dev(get(name + ".bias"))

        def resnet(p, c_in, c_out):
            r = _Resnet()
            r.n1, r.c1 = norm(p + "norm1", c_in), conv(p + "conv1", c_out, c_in, 3)
            r.n2, r.c2 = norm(p + "norm2", c_out), conv(p + "conv2", c_out, c_out, 3)
            r.shortcut = conv(p + "conv_shortcut", c_out, c_in, 1) if c_in != c_out else None
            return r

        lc, top = spec.latent_channels, spec.block_out_channels[-1]
        self.post_quant = conv("post_quant_conv", lc, lc, 1) if has("post_quant_conv.weight") else None
        self.conv_in = conv("decoder.conv_in", top, lc, 3)
        self.mid = [resnet("decoder.mid_block.resnets.0.", top, top), resnet("decoder.mid_block.resnets.1.", top, top)]
        a = "decoder.mid_block.attentions.0."
        self.attn_norm = norm(a + "group_norm", top)
        s = 1.0 / np.sqrt(np.float32(top))
        wq, wk, wv, wo = (get(a + n + ".weight").reshape(top, top) for n in ("to_q", "to_k", "to_v", "to_out.0"))
        bq, bk, bv, bo = (get(a + n + ".bias") for n in ("to_q", "to_k", "to_v", "to_out.0"))
        wq, bq = (wq * s).astype(np.float32), (bq * s).astype(np.float32)
        self.q_w, self.q_b, self.k_w, self.k_b = dev(wq), dev(bq), dev(wk), dev(bk)
        self.v_w = dev(wv)
        self.qkv_w, self.qkv_b = dev(np.concatenate([wq, wk, wv])), dev(np.concatenate([bq, bk, np.zeros_like(bv)]))
        self.out_w = dev(wo)
        self.out_b = dev((wo.astype(np.float64) @ bv.astype(np.float64) + bo).astype(np.float32))
        self.channels = top
        self.up = []
        for i, (c_in, c_out, up) in enumerate(_up_blocks(spec)):
            p = f"decoder.up_blocks.{i}."
            rs = [resnet(p + f"resnets.{j}.", c_in if j == 0 else c_out, c_out) for j in range(spec.layers_per_block + 1)]
            self.up.append((rs, conv(p + "upsamplers.0.conv", c_out, c_out, 3) if up else None))
        c0 = spec.block_out_channels[0]
        self.norm_out = norm("decoder.conv_norm_out", c0)
        self.conv_out = conv("decoder.conv_out", spec.out_channels, c0, 3)
        self._consts: dict = {}
        self._const_shape: tuple = ()

    # ------------------------------------------------------------------ loading
    @staticmethod
    def find_safetensors(path) -> Path:
        """A file as it is; in a directory vae.safetensors, diffusion_pytorch_model.safetensors, the first *vae*.safetensors, the
        first *.safetensors (the reference's search order)."""
        path = Path(path)
        if not path.is_dir():
            return path
        for name in ("vae.safetensors", "diffusion_pytorch_model.safetensors"):
            if (path / name).exists():
                return path / name
        found = sorted(path.glob("*vae*.safetensors")) or sorted(path.glob("*.safetensors"))
        if not found:
            raise FileNotFoundError(f"No safetensors file found in {path}")
        return found[0]

    @classmethod
    def read_safetensors(cls, path, spec: "VAESpec | None" = None) -> "tuple[VAESpec, dict]":
        """Host side of from_safetensors, no device: (spec, {name: float32 array}) with the encoder's tensors and the encoder-side
        quant_conv left out.  Without a spec: 16 latent channels (decoder.conv_in's input) -> SD3_VAE_SPEC, else SDXL_VAE_SPEC."""
        from pygpukit_amd.llm.safetensors import load_safetensors

        st = load_safetensors(str(cls.find_safetensors(path)))

        def wanted(name):
            parts = name.split(".")
            return "encoder" not in parts and "quant_conv" not in parts

        weights = {name: st.tensor_as_f32(name) for name in st.tensor_names if wanted(name)}
        if spec is None:
            key = next((k for k in weights if k.endswith("decoder.conv_in.weight")), None)
            spec = SD3_VAE_SPEC if key is not None and weights[key].shape[1] == 16 else SDXL_VAE_SPEC
        return spec, weights

    @classmethod
    def from_safetensors(cls, path, spec: "VAESpec | None" = None, dtype: "str | DataType" = "float32", attention: str = "auto") -> "VAE":
        """find_safetensors(path), read_safetensors, upload."""
        spec, weights = cls.read_safetensors(path, spec)
        return cls(spec, weights, dtype=dtype, attention=attention)

    # ------------------------------------------------------------------ pieces
    def _const(self, value: float, shape) -> GPUArray:
        """A float32 array of the latent's shape filled with `value` (the elementwise ops take arrays).  Kept for the LAST latent
        shape only, so a caller that varies the resolution does not accumulate them."""
        if self._const_shape != tuple(shape):
            self._consts, self._const_shape = {}, tuple(shape)
        if value not in self._consts:
            self._consts[value] = from_numpy(np.full(shape, value, np.float32))
        return self._consts[value]

    def _resnet(self, r: _Resnet, x: GPUArray) -> GPUArray:
        h = r.c1(group_norm_silu(x, *r.n1, self.groups, self.eps, channels_last=True))
        group_norm_silu(h, *r.n2, self.groups, self.eps, channels_last=True, out=h)
        return r.c2(h, add=r.shortcut(x) if r.shortcut is not None else x)

    def _attention(self, x: GPUArray, path: str) -> GPUArray:
        B, H, W, C = x.shape
        T = H * W
        rows = group_norm(x, *self.attn_norm, self.groups, self.eps, channels_last=True)._view(0, (B * T, C))
        o = GPUArray((B * T, C), self.dtype)
        if path == "sdpa":
            qkv = matmul_nt(rows, self.qkv_w, self.qkv_b)                                   # [B T, 3 C]: q | k | v per row
            for b in range(B):
                base = b * T * 3 * C
                sdpa_noncausal_strided(qkv._view(base, (qkv.size - base,)), qkv._view(base + C, (qkv.size - base - C,)),
                                       qkv._view(base + 2 * C, (qkv.size - base - 2 * C,)), o._view(b * T * C, (T, C)), 1, 1, T, T, C,
                                       (C, 3 * C), (C, 3 * C), (C, C), 1.0)
        else:
            q, k = matmul_nt(rows, self.q_w, self.q_b), matmul_nt(rows, self.k_w, self.k_b)
            for b in range(B):
                xb = rows._view(b * T * C, (T, C))
                vt = matmul_nt(self.v_w, xb)                                                # [C, T] = W_v X^T: V transposed, no bias
                p = softmax(matmul_nt(q._view(b * T * C, (T, C)), k._view(b * T * C, (T, C))))   # [T, T]
                matmul_nt(p, vt, out=o._view(b * T * C, (T, C)))
        y = matmul_nt(o, self.out_w, self.out_b)
        xr = x._view(0, (B * T, C))
        return add(y, xr, out=y)._view(0, (B, H, W, C))

    # ------------------------------------------------------------------ decode
    def decode(self, latent: GPUArray) -> GPUArray:
        lc = self.spec.latent_channels
        if latent.ndim != 4 or latent.shape[1] != lc or 0 in latent.shape:
            raise ValueError(f"VAE.decode: latent must be [B, {lc}, H, W], got {latent.shape}")
        B, _, H, W = latent.shape
        path = vae_plan(self.spec, self.dtype, (H, W), self.attention, self.post_quant is not None, B)["attention"]
        x = latent.astype(float32)
        x = div(x, self._const(self.spec.scaling_factor, x.shape))
        if self.spec.shift_factor != 0.0:
            x = add(x, self._const(self.spec.shift_factor, x.shape), out=x)
        x = x.astype(self.dtype)
        if self.post_quant is not None:
            x = self.post_quant(x, cl_in=False, cl_out=False)
        x = self.conv_in(x, cl_in=False)                                                    # channels-last from here on
        x = self._resnet(self.mid[0], x)
        x = self._attention(x, path)
        x = self._resnet(self.mid[1], x)
        for resnets, upsampler in self.up:
            for r in resnets:
                x = self._resnet(r, x)
            if upsampler is not None:
                x = upsampler(x, upsample=2)
        group_norm_silu(x, *self.norm_out, self.groups, self.eps, channels_last=True, out=x)
        return clamp(self.conv_out(x, cl_out=False), -1.0, 1.0)

    def encode(self, image: GPUArray) -> GPUArray:
        raise NotImplementedError("VAE.encode: the encoder is not built (the reference's is a placeholder that averages 8x8 blocks)")

    def to_pil(self, image: GPUArray):
        """[B, 3, H, W] in [-1, 1] -> a PIL image (a list of them for B > 1), as the reference."""
        x = image.astype(float32).to_numpy()
        if x.ndim == 4:
            if x.shape[0] != 1:
                return [self._array_to_pil(x[i]) for i in range(x.shape[0])]
            x = x[0]
        return self._array_to_pil(x)

    @staticmethod
    def _array_to_pil(x: np.ndarray):
        from PIL import Image

        return Image.fromarray(((x.transpose(1, 2, 0) + 1) * 127.5).clip(0, 255).astype(np.uint8))


__all__ = ["VAE", "vae_plan", "SDPA_MAX_KEYS"]
