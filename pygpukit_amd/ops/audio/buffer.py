"""AudioBuffer, from_pcm and the sample-domain ops (reference: src/pygpukit/ops/audio/buffer.py over native/ops/audio/audio.cu).
Each op is one launch of csrc/ops_audio.hip on float32; the reference's normalize ops run two kernels around a host reduction."""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import float32, int16
from pygpukit_amd.core.factory import from_numpy
from pygpukit_amd.ops._common import call
from pygpukit_amd.ops.audio import tables

_OP_PCM, _OP_MONO = 0, 1
_taps: dict[int, GPUArray] = {}


def _f32(a: GPUArray, name: str) -> None:
    if a.dtype != float32:
        raise ValueError(f"{name}: input must be float32, got {a.dtype}")


def pcm_to_float32(samples: GPUArray) -> GPUArray:
    """int16 -> x / 32768 (float32, exact)."""
    if samples.dtype != int16:
        raise ValueError(f"pcm_to_float32: input must be int16, got {samples.dtype}")
    out = GPUArray(samples.shape, float32)
    call("pgk_audio_map", samples._p, out._p, samples.size, _OP_PCM, 0.0, None)
    return out


def stereo_to_mono(samples: GPUArray) -> GPUArray:
    """Interleaved L R L R ... -> (l + r) * 0.5."""
    _f32(samples, "stereo_to_mono")
    if samples.size % 2:
        raise ValueError(f"stereo_to_mono: interleaved stereo needs an even number of samples, got {samples.size}")
    out = GPUArray((samples.size // 2,), float32)
    call("pgk_audio_map", samples._p, out._p, out.size, _OP_MONO, 0.0, None)
    return out


def normalize_peak(samples: GPUArray) -> None:
    """In place: x / max|x| when the peak exceeds 1e-8."""
    _f32(samples, "normalize_peak")
    call("pgk_audio_normalize", samples._p, samples.size, 0, 0.0, None)


def normalize_rms(samples: GPUArray, target_db: float = -20.0) -> None:
    """In place: x * 10^(target_db / 20) / rms(x) when the rms exceeds 1e-8."""
    _f32(samples, "normalize_rms")
    call("pgk_audio_normalize", samples._p, samples.size, 1, float(10.0 ** (float(target_db) / 20.0)), None)


def resample(samples: "GPUArray | np.ndarray | AudioBuffer", src_rate: int, dst_rate: int) -> GPUArray:
    """n * dst // src output samples.  src % dst == 0: a Kaiser windowed-sinc decimator designed on the host
    (tables.decimator_taps); otherwise linear interpolation with the position computed in integers.  src == dst: a copy."""
    if isinstance(samples, AudioBuffer):
        samples = samples.data
    if isinstance(samples, np.ndarray):
        samples = from_numpy(np.ascontiguousarray(samples, dtype=np.float32))
    _f32(samples, "resample")
    src, dst = int(src_rate), int(dst_rate)
    if samples.ndim != 1 or not 1 <= src < 2 ** 31 or not 1 <= dst < 2 ** 31:
        raise ValueError(f"resample: needs 1-D samples and positive rates, got shape {samples.shape}, {src_rate} -> {dst_rate}")
    if src == dst:
        return samples.clone()
    n = samples.size
    out = GPUArray((tables.resampled_length(n, src, dst),), float32)
    if n == 0 or out.size == 0:
        return out
    ratio = src // dst if src % dst == 0 else 0
    taps = None
    if ratio:
        if ratio not in _taps:
            _taps[ratio] = from_numpy(tables.decimator_taps(ratio))
        taps = _taps[ratio]
    call("pgk_audio_resample", samples._p, out._p, taps._p if taps is not None else None, n, out.size, ratio,
         taps.size if taps is not None else 0, src, dst, None)
    return out


@dataclass
class AudioBuffer:
    """Samples on the device (float32) with their sample rate and channel count (2 = interleaved stereo)."""

    data: GPUArray
    sample_rate: int
    channels: int

    def to_mono(self) -> "AudioBuffer":
        if self.channels == 1:
            return self
        if self.channels != 2:
            raise ValueError(f"to_mono only supports stereo (2 channels), got {self.channels}")
        return AudioBuffer(data=stereo_to_mono(self.data), sample_rate=self.sample_rate, channels=1)

    def resample(self, target_rate: int) -> "AudioBuffer":
        if self.sample_rate == target_rate:
            return self
        if self.channels != 1:
            raise ValueError(f"resample needs mono audio (call to_mono() first), got {self.channels} channels")
        return AudioBuffer(data=resample(self.data, self.sample_rate, target_rate), sample_rate=target_rate, channels=self.channels)

    def normalize(self, mode: str = "peak", target_db: float = -20.0) -> "AudioBuffer":
        if mode == "peak":
            normalize_peak(self.data)
        elif mode == "rms":
            normalize_rms(self.data, target_db)
        else:
            raise ValueError(f"Unknown normalization mode: {mode}. Use 'peak' or 'rms'.")
        return self

    def to_numpy(self) -> np.ndarray:
        return self.data.to_numpy()

    def __repr__(self) -> str:
        return f"AudioBuffer(samples={self.data.shape[0]}, sample_rate={self.sample_rate}, channels={self.channels})"


def from_pcm(samples: "np.ndarray | GPUArray", sample_rate: int, channels: int = 1) -> AudioBuffer:
    """int16 PCM (converted on the device) or float32 samples -> AudioBuffer."""
    if isinstance(samples, np.ndarray):
        if samples.dtype not in (np.int16, np.float32):
            raise ValueError(f"Unsupported dtype: {samples.dtype}. Use int16 or float32.")
        samples = from_numpy(samples)
    if samples.dtype == int16:
        data = pcm_to_float32(samples)
    elif samples.dtype == float32:
        data = samples
    else:
        raise ValueError(f"Unsupported dtype: {samples.dtype}. Use int16 or float32.")
    return AudioBuffer(data=data, sample_rate=sample_rate, channels=channels)


__all__ = ["AudioBuffer", "from_pcm", "pcm_to_float32", "stereo_to_mono", "normalize_peak", "normalize_rms", "resample"]
