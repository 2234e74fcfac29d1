"""Diffusion-specific operations (reference: src/pygpukit/diffusion/ops).  `__all__` starts with the reference's list minus
group_norm, conv2d and conv2d_transpose: those belong to the VAE, which is out of scope here.  Added to it: the native-only ops of
the reference's diffusion.inl (layer_norm_simple, modulate, gated_residual), the names its sub-modules export (modulation,
self_attention, timestep_mlp), this build's own gated_residual_adaln, adaln_plan, Modulation, patchify and unpatchify, and the
FLUX row ops (flux_qk_norm_rope and its plan, flux_gelu_pack, flux_unpack_latents, flow_euler_step)."""

from __future__ import annotations

from pygpukit_amd.diffusion.ops.adaln import (Modulation, adaln, adaln_plan, adaln_zero, gated_residual, gated_residual_adaln,
                                              layer_norm_simple, modulate, modulation)
from pygpukit_amd.diffusion.ops.cross_attention import cross_attention, self_attention
from pygpukit_amd.diffusion.ops.flux import (flow_euler_step, flux_gelu_pack, flux_qk_norm_rope, flux_qk_norm_rope_plan,
                                             flux_unpack_latents)
from pygpukit_amd.diffusion.ops.patch import patchify, unpatchify
from pygpukit_amd.diffusion.ops.timestep_embed import sinusoidal_timestep_embedding, timestep_mlp

__all__ = [
    "cross_attention",
    "sinusoidal_timestep_embedding",
    "adaln",
    "adaln_zero",
    "self_attention",
    "timestep_mlp",
    "modulation",
    "layer_norm_simple",
    "modulate",
    "gated_residual",
    "gated_residual_adaln",
    "adaln_plan",
    "Modulation",
    "patchify",
    "unpatchify",
    "flux_qk_norm_rope",
    "flux_qk_norm_rope_plan",
    "flux_gelu_pack",
    "flux_unpack_latents",
    "flow_euler_step",
]
