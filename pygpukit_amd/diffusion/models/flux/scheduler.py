"""Flow-matching Euler scheduler of FLUX (reference: src/pygpukit/diffusion/models/flux/scheduler.py): the same methods and the
same numbers.  x_t = (1 - sigma) x_0 + sigma noise with sigma from 1 to 0; the model predicts the velocity and a step is
x += (sigma_next - sigma) * v.  `step` takes NumPy arrays as the reference's does, and also a float32 GPUArray sample with a
GPUArray model output in any float dtype, which is one launch of flow_euler_step on the sample in place."""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np


@dataclass
class FlowMatchEulerSchedulerConfig:
    num_train_timesteps: int = 1000
    shift: float = 1.0
    use_dynamic_shifting: bool = False
    base_shift: float = 0.5
    max_shift: float = 1.15
    base_image_seq_len: int = 256
    max_image_seq_len: int = 4096


class FlowMatchEulerScheduler:
    def __init__(self, config: "FlowMatchEulerSchedulerConfig | None" = None):
        self.config = config or FlowMatchEulerSchedulerConfig()
        self.num_inference_steps: "int | None" = None
        self.timesteps: "np.ndarray | None" = None
        self.sigmas: "np.ndarray | None" = None
        self._step_index: "int | None" = None

    def set_timesteps(self, num_inference_steps: int, mu: "float | None" = None) -> None:
        """sigmas [steps + 1] float32: linear from 1 to 0 in float64, warped by shift * s / (1 + (shift - 1) * s) when shift != 1,
        then by the exponential time shift when dynamic shifting is on and mu is given; timesteps = sigmas[:-1] * num_train_timesteps."""
        self.num_inference_steps = num_inference_steps
        s = np.linspace(1.0, 0.0, num_inference_steps + 1)
        shift = self.config.shift
        if shift != 1.0:
            s = shift * s / (1.0 + (shift - 1.0) * s)
        if self.config.use_dynamic_shifting and mu is not None:
            s = self._time_shift(mu, 1.0, s)
        self.sigmas = s.astype(np.float32)
        self.timesteps = (self.sigmas[:-1] * self.config.num_train_timesteps).astype(np.float32)
        self._step_index = 0

    def _time_shift(self, mu: float, sigma: float, t: np.ndarray) -> np.ndarray:
        return np.exp(mu) / (np.exp(mu) + (1 / t - 1) ** sigma)

    def compute_mu(self, image_seq_len: int) -> float:
        """The line through (base_image_seq_len, base_shift) and (max_image_seq_len, max_shift) at image_seq_len."""
        c = self.config
        m = (c.max_shift - c.base_shift) / (c.max_image_seq_len - c.base_image_seq_len)
        b = c.base_shift - m * c.base_image_seq_len
        return image_seq_len * m + b

    @property
    def step_index(self) -> "int | None":
        return self._step_index

    def step(self, model_output, timestep, sample):
        """One Euler step from the current sigma to the next; `timestep` is not used (the reference's signature)."""
        if self._step_index is None or self.sigmas is None:
            raise ValueError("Timesteps not set. Call set_timesteps() first.")
        dt = self.sigmas[self._step_index + 1] - self.sigmas[self._step_index]
        from pygpukit_amd.core.array import GPUArray

        if isinstance(sample, GPUArray) or isinstance(model_output, GPUArray):
            if not (isinstance(sample, GPUArray) and isinstance(model_output, GPUArray)):
                raise ValueError("FlowMatchEulerScheduler.step: sample and model_output must both be GPUArrays or both NumPy arrays")
            from pygpukit_amd.diffusion.ops.flux import flow_euler_step

            prev = flow_euler_step(sample, model_output, float(dt))
        else:
            prev = (sample + dt * model_output).astype(np.float32)
        self._step_index += 1
        return prev

    def add_noise(self, original_samples: np.ndarray, noise: np.ndarray, timestep: float) -> np.ndarray:
        return ((1.0 - timestep) * original_samples + timestep * noise).astype(np.float32)

    def scale_model_input(self, sample, timestep=None):
        return sample


__all__ = ["FlowMatchEulerScheduler", "FlowMatchEulerSchedulerConfig"]
