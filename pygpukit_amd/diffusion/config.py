"""Architecture descriptions of the diffusion transformers (reference: src/pygpukit/diffusion/config.py: the DiTSpec / PixArtSpec
field names and PIXART_SIGMA_SPEC's values, VAESpec and the three VAE specs; the SD3 and Flux transformer specs belong to models
this package does not build yet)."""

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


@dataclass(frozen=True)
class VAESpec:
    """The reference's fields and defaults, plus shift_factor [build-defined]: decode computes latent / scaling_factor +
    shift_factor (diffusers' SD3 and Flux VAEs carry one; 0.0 reproduces the reference)."""
    name: str
    in_channels: int = 3
    out_channels: int = 3
    latent_channels: int = 4
    scaling_factor: float = 0.18215   # SD 1.5
    block_out_channels: "tuple[int, ...]" = (128, 256, 512, 512)
    layers_per_block: int = 2
    norm_num_groups: int = 32
    norm_eps: float = 1e-6
    shift_factor: float = 0.0


SDXL_VAE_SPEC = VAESpec(name="sdxl_vae", latent_channels=4, scaling_factor=0.13025, block_out_channels=(128, 256, 512, 512))
SD3_VAE_SPEC = VAESpec(name="sd3_vae", latent_channels=16, scaling_factor=1.5305, block_out_channels=(128, 256, 512, 512))
FLUX_VAE_SPEC = VAESpec(name="flux_vae", latent_channels=16, scaling_factor=0.3611, block_out_channels=(128, 256, 512, 512))

__all__ = ["DiTSpec", "PixArtSpec", "PIXART_SIGMA_SPEC", "VAESpec", "SDXL_VAE_SPEC", "SD3_VAE_SPEC", "FLUX_VAE_SPEC"]
