"""Diffusion models (reference: src/pygpukit/diffusion).  Built so far: the DiT transformer path - diffusion.ops and
models.dit.PixArtTransformer - the VAE decoder, models.vae.VAE, on pygpukit_amd.ops.conv2d / group_norm / group_norm_silu
(they live in pygpukit_amd.ops, not in diffusion.ops: INTEGRATION.md), and FLUX: models.flux.FluxTransformer, its flow-matching
Euler scheduler and FluxPipeline on precomputed text embeddings or, given the two encoders, on a prompt; text_encoders: the T5 and
CLIP text encoders.  The VAE encoder, conv2d_transpose and the reference's other schedulers are not."""

from pygpukit_amd.diffusion.config import (FLUX_VAE_SPEC, PIXART_SIGMA_SPEC, SD3_VAE_SPEC, SDXL_VAE_SPEC, DiTSpec, PixArtSpec,
                                           VAESpec)
from pygpukit_amd.diffusion.models.dit import PixArtTransformer, dit_plan
from pygpukit_amd.diffusion.models.flux import (FlowMatchEulerScheduler, FlowMatchEulerSchedulerConfig, FluxConfig, FluxPipeline,
                                                FluxTransformer, flux_plan)
from pygpukit_amd.diffusion.models.vae import VAE, vae_plan
from pygpukit_amd.diffusion.text_encoders import CLIPTextEncoder, CLIPTextEncoderG, CLIPTextEncoderL, T5Encoder, T5XXLEncoder, t5_plan

__all__ = ["DiTSpec", "PixArtSpec", "PIXART_SIGMA_SPEC", "PixArtTransformer", "dit_plan", "VAE", "VAESpec", "SDXL_VAE_SPEC",
           "SD3_VAE_SPEC", "FLUX_VAE_SPEC", "vae_plan", "FluxTransformer", "FluxConfig", "FluxPipeline", "FlowMatchEulerScheduler",
           "FlowMatchEulerSchedulerConfig", "flux_plan", "T5Encoder", "T5XXLEncoder", "CLIPTextEncoder", "CLIPTextEncoderL",
           "CLIPTextEncoderG", "t5_plan"]
