"""Diffusion model implementations (reference: src/pygpukit/diffusion/models): the DiT family's PixArtTransformer and the VAE decoder."""

from pygpukit_amd.diffusion.models.dit import PixArtTransformer, dit_plan
from pygpukit_amd.diffusion.models.vae import VAE, vae_plan

__all__ = ["PixArtTransformer", "dit_plan", "VAE", "vae_plan"]
