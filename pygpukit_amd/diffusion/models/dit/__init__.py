"""DiT (diffusion transformer) models (reference: src/pygpukit/diffusion/models/dit): PixArtTransformer.  The reference's DiT /
SD3Transformer / FluxTransformer bases are not built."""

from pygpukit_amd.diffusion.models.dit.embeddings import get_2d_sincos_pos_embed, sinusoidal_embedding
from pygpukit_amd.diffusion.models.dit.model import PixArtTransformer, dit_plan, pack_head_columns, pack_head_rows

__all__ = ["PixArtTransformer", "dit_plan", "pack_head_rows", "pack_head_columns", "sinusoidal_embedding", "get_2d_sincos_pos_embed"]
