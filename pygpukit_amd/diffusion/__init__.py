"""Diffusion models (reference: src/pygpukit/diffusion).  Built so far: the DiT transformer path - diffusion.ops and
models.dit.PixArtTransformer.  The VAE (group_norm, conv2d), Flux, the text encoders, the schedulers and the pipeline are not."""

from pygpukit_amd.diffusion.config import PIXART_SIGMA_SPEC, DiTSpec, PixArtSpec
from pygpukit_amd.diffusion.models.dit import PixArtTransformer, dit_plan

__all__ = ["DiTSpec", "PixArtSpec", "PIXART_SIGMA_SPEC", "PixArtTransformer", "dit_plan"]
