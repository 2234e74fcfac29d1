"""Architecture descriptions of the diffusion transformers (reference: src/pygpukit/diffusion/config.py: the DiTSpec / PixArtSpec
field names and PIXART_SIGMA_SPEC's values; SD3, Flux and the VAE specs belong to models this package does not build yet)."""

from __future__ import annotations

from dataclasses import dataclass


@dataclass(frozen=True)
class DiTSpec:
    name: str
    hidden_size: int
    num_layers: int
    num_heads: int
    conditioning_type: str            # "adaln" | "adaln_zero" | "cross_attn"
    text_encoder_dim: int
    pos_embed_type: str               # "sinusoidal" | "rope_2d" | "learned"
    patch_size: int = 2
    in_channels: int = 16
    out_channels: int = 16
    is_mmdit: bool = False
    mlp_ratio: float = 4.0
    head_dim: "int | None" = None

    def get_head_dim(self) -> int:
        return self.head_dim if self.head_dim is not None else self.hidden_size // self.num_heads


@dataclass(frozen=True)
class PixArtSpec(DiTSpec):
    cross_attention_dim: int = 4096   # T5-XXL


PIXART_SIGMA_SPEC = PixArtSpec(name="pixart_sigma", hidden_size=1152, num_layers=28, num_heads=16, conditioning_type="cross_attn",
                               text_encoder_dim=4096, pos_embed_type="sinusoidal", in_channels=4, out_channels=8,
                               cross_attention_dim=4096)

__all__ = ["DiTSpec", "PixArtSpec", "PIXART_SIGMA_SPEC"]
