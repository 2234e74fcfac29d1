"""Diffusion model implementations (reference: src/pygpukit/diffusion/models): the DiT family's PixArtTransformer, the VAE decoder
and the FLUX transformer with its scheduler and pipeline."""

from pygpukit_amd.diffusion.models.dit import PixArtTransformer, dit_plan
from pygpukit_amd.diffusion.models.flux import (FlowMatchEulerScheduler, FlowMatchEulerSchedulerConfig, FluxConfig, FluxPipeline,
                                                FluxTransformer, flux_plan)
from pygpukit_amd.diffusion.models.vae import VAE, vae_plan

__all__ = ["PixArtTransformer", "dit_plan", "VAE", "vae_plan", "FluxTransformer", "FluxConfig", "FluxPipeline",
           "FlowMatchEulerScheduler", "FlowMatchEulerSchedulerConfig", "flux_plan"]
