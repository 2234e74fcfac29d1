"""FLUX generation loop (reference: src/pygpukit/diffusion/models/flux/pipeline.py) on precomputed text embeddings: noise is drawn
once on the host, then transformer -> scheduler step -> unpack -> VAE.decode all stay on the device.  The text encoders (T5,
CLIP) and their tokenisers are not built, so a string prompt, encode_prompt and from_pretrained raise and point at prompt_embeds."""

from __future__ import annotations

import numpy as np

from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import float32
from pygpukit_amd.core.factory import from_numpy
from pygpukit_amd.diffusion.models.flux.embeddings import prepare_image_ids, prepare_text_ids
from pygpukit_amd.diffusion.models.flux.model import FluxTransformer
from pygpukit_amd.diffusion.models.flux.scheduler import FlowMatchEulerScheduler, FlowMatchEulerSchedulerConfig
from pygpukit_amd.diffusion.ops.flux import flux_unpack_latents
from pygpukit_amd.diffusion.ops.patch import patchify

_NO_ENCODERS = ("the T5 / CLIP text encoders are not built: pass prompt_embeds [B, tokens, joint_attention_dim] and "
                "pooled_prompt_embeds [B, pooled_projection_dim] computed elsewhere")


class FluxPipeline:
    """pipe(prompt_embeds, pooled_prompt_embeds, height, width) -> image GPUArray [B, 3, height, width] in [-1, 1]."""

    def __init__(self, transformer: FluxTransformer, vae, scheduler: "FlowMatchEulerScheduler | None" = None):
        self.transformer = transformer
        self.vae = vae
        self.scheduler = scheduler or FlowMatchEulerScheduler(FlowMatchEulerSchedulerConfig())
        self.vae_scale_factor = 16                                  # 8x VAE and 2x2 packing
        self.latent_channels = transformer.config.in_channels       # after packing: 4 x the VAE's latent channels
        if self.latent_channels % 4:
            raise ValueError(f"FluxPipeline: {self.latent_channels} packed channels are no multiple of 4")

    @classmethod
    def from_pretrained(cls, path, dtype: str = "float32"):
        raise NotImplementedError(f"FluxPipeline.from_pretrained: {_NO_ENCODERS}; build the pipeline from FluxTransformer.from_safetensors "
                                  "and VAE.from_safetensors")

    def encode_prompt(self, prompt, max_sequence_length: int = 512):
        raise NotImplementedError(f"FluxPipeline.encode_prompt: {_NO_ENCODERS}")

    # ------------------------------------------------------------------ latent packing
    @staticmethod
    def pack_latents(latents: GPUArray) -> GPUArray:
        """[B, C, 2h, 2w] -> [B, h * w, C * 4] with columns (c, ph, pw): patchify(x, 2), reshaped."""
        B, C, H, W = latents.shape
        return patchify(latents, 2)._view(0, (B, (H // 2) * (W // 2), C * 4))

    def unpack_latents(self, latents: GPUArray, height: int, width: int) -> GPUArray:
        """[B, h * w, C * 4] -> [B, C, height / 8, width / 8] for an image of height x width."""
        return flux_unpack_latents(latents, height // self.vae_scale_factor, width // self.vae_scale_factor)

    _unpack_latents = unpack_latents

    def decode_latents(self, latents: GPUArray, height: int, width: int) -> GPUArray:
        """Packed latents -> image [B, 3, height, width] in [-1, 1] (VAE.decode applies scaling_factor and shift_factor)."""
        return self.vae.decode(self.unpack_latents(latents, height, width))

    @staticmethod
    def to_uint8(image: GPUArray) -> np.ndarray:
        """[B, 3, H, W] in [-1, 1] -> uint8 [B, H, W, 3], the reference's decode_latents conversion."""
        x = (image.astype(float32).to_numpy() + 1.0) / 2.0
        return np.clip(x * 255, 0, 255).astype(np.uint8).transpose(0, 2, 3, 1)

    # ------------------------------------------------------------------ generation
    def __call__(self, prompt_embeds=None, pooled_prompt_embeds=None, height: int = 512, width: int = 512, num_inference_steps: int = 4,
                 guidance_scale: float = 0.0, seed: "int | None" = None, latents=None, prompt=None) -> GPUArray:
        if isinstance(prompt_embeds, str) or prompt is not None:
            raise NotImplementedError(f"FluxPipeline: {_NO_ENCODERS}")
        if prompt_embeds is None or pooled_prompt_embeds is None:
            raise ValueError("FluxPipeline: prompt_embeds and pooled_prompt_embeds are required")
        if height % 16 or width % 16:
            raise ValueError(f"Height and width must be divisible by 16, got {height}x{width}")
        embeds, pooled = (a if isinstance(a, GPUArray) else from_numpy(np.ascontiguousarray(a, dtype=np.float32))
                          for a in (prompt_embeds, pooled_prompt_embeds))
        B = embeds.shape[0]
        lh, lw = height // self.vae_scale_factor, width // self.vae_scale_factor
        tokens = lh * lw
        img_ids = prepare_image_ids(1, lh, lw)
        txt_ids = prepare_text_ids(1, embeds.shape[1])
        if latents is None:
            latents = np.random.default_rng(seed).standard_normal((B, tokens, self.latent_channels)).astype(np.float32)
        if not isinstance(latents, GPUArray):
            latents = from_numpy(np.ascontiguousarray(latents, dtype=np.float32))
        if latents.shape != (B, tokens, self.latent_channels) or latents.dtype != float32:
            raise ValueError(f"FluxPipeline: latents must be float32 {(B, tokens, self.latent_channels)}, got {latents.shape} {latents.dtype.name}")
        latents = latents.clone()                                   # stepped in place
        self.transformer.set_encoder_states(embeds, pooled)
        guidance = np.full(B, guidance_scale, np.float32) if self.transformer.config.guidance_embeds else None
        self.scheduler.set_timesteps(num_inference_steps)
        for t in self.scheduler.timesteps:
            v = self.transformer.forward(latents, timestep=np.full(B, t, np.float32), img_ids=img_ids, txt_ids=txt_ids, guidance=guidance)
            latents = self.scheduler.step(v, t, latents)
        return self.decode_latents(latents, height, width)


__all__ = ["FluxPipeline"]
