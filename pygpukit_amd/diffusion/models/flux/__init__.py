"""FLUX.1 rectified-flow transformer (reference: src/pygpukit/diffusion/models/flux).  The reference's names, so that host code
written against it imports unchanged; `generate` is absent with the text encoders it needs, and flux_plan is this build's own."""

from __future__ import annotations

from pygpukit_amd.diffusion.models.flux.model import FluxConfig, FluxTransformer, flux_plan
from pygpukit_amd.diffusion.models.flux.pipeline import FluxPipeline
from pygpukit_amd.diffusion.models.flux.scheduler import FlowMatchEulerScheduler, FlowMatchEulerSchedulerConfig

__all__ = [
    "FluxTransformer",
    "FluxConfig",
    "FlowMatchEulerScheduler",
    "FlowMatchEulerSchedulerConfig",
    "FluxPipeline",
    "flux_plan",
]
