"""FLUX generation loop (reference: src/pygpukit/diffusion/models/flux/pipeline.py) on precomputed text embeddings: noise is drawn
once on the host, then transformer -> scheduler step -> unpack -> VAE.decode all stay on the device.  Given text_encoder= (a
CLIPTextEncoder) and text_encoder_2= (a T5Encoder), encode_prompt and a string prompt work; without them they raise and point at
prompt_embeds, as from_pretrained always does (hub layouts and downloads are out of scope)."""

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

_NO_ENCODERS = ("no T5 / CLIP text encoders were given (text_encoder=, text_encoder_2=): pass prompt_embeds [B, tokens, joint_attention_dim] and "
                "pooled_prompt_embeds [B, pooled_projection_dim] computed elsewhere")


class FluxPipeline:
    """pipe(prompt_embeds, pooled_prompt_embeds, height, width) -> image GPUArray [B, 3, height, width] in [-1, 1]."""

    def __init__(self, transformer: FluxTransformer, vae, scheduler: "FlowMatchEulerScheduler | None" = None, *, text_encoder=None,
                 text_encoder_2=None):
        self.transformer = transformer
        self.text_encoder = text_encoder            # CLIP: pooled_prompt_embeds
        self.text_encoder_2 = text_encoder_2        # T5: prompt_embeds
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

    def _has_encoders(self) -> bool:
        return getattr(self, "text_encoder", None) is not None and getattr(self, "text_encoder_2", None) is not None

    def encode_prompt(self, prompt, max_sequence_length: int = 512, *, mask_padding: bool = True):
        """-> (pooled [B, pooled_projection_dim], t5_embeds [B, max_sequence_length, joint_attention_dim]), the reference's order.
        CLIP is padded / truncated to 77 tokens, T5 to max_sequence_length.  mask_padding=True keeps T5's padding out of its
        attention (the reference's mask); False attends it, as diffusers' FluxPipeline does."""
        if not self._has_encoders():
            raise NotImplementedError(f"FluxPipeline.encode_prompt: {_NO_ENCODERS}")
        clip_ids, clip_mask = self.text_encoder.tokenize(prompt, max_length=77)
        _, pooled = self.text_encoder.forward(clip_ids, clip_mask)
        t5_ids, t5_mask = self.text_encoder_2.tokenize(prompt, max_length=max_sequence_length)
        return pooled, self.text_encoder_2.forward(t5_ids, t5_mask if mask_padding else None)

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
        is_text = isinstance(prompt_embeds, str) or (isinstance(prompt_embeds, (list, tuple)) and len(prompt_embeds) > 0
                                                     and all(isinstance(p, str) for p in prompt_embeds))
        if is_text and prompt is None:              # the reference's first positional argument is the prompt
            prompt, prompt_embeds = prompt_embeds, None
        if prompt is not None:
            if not self._has_encoders():
                raise NotImplementedError(f"FluxPipeline: {_NO_ENCODERS}")
            pooled_prompt_embeds, prompt_embeds = self.encode_prompt(prompt)
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
