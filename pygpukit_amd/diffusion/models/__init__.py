"""Diffusion model implementations (reference: src/pygpukit/diffusion/models): the DiT family's PixArtTransformer."""

from pygpukit_amd.diffusion.models.dit import PixArtTransformer, dit_plan

__all__ = ["PixArtTransformer", "dit_plan"]
