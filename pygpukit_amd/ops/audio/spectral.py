"""Spectral ops (reference: src/pygpukit/ops/audio/spectral.py over native/ops/audio/audio.cu).

log_mel_features is the fused kernel of csrc/ops_audio.hip: samples -> windowed frames -> DFT on the f32 MFMA -> power ->
filterbank -> log -> affine -> cast, one launch (two kernels when dynamic_range is given).  mel_spectrogram and
log_mel_spectrogram call it; stft, power_spectrum, magnitude_spectrum, apply_mel_filterbank, log_mel and to_decibels are the
reference's unfused steps, one launch each.  Semantics are the reference's CUDA ones (periodic Hann, HTK mel triangles evaluated in
Hz); differences: any even n_fft in [16, 2048] is accepted, and stft's output really is interleaved."""

from __future__ import annotations

import math

import numpy as np

from pygpukit_amd import _hip
from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import DataType, as_dtype, float32, int32
from pygpukit_amd.core.factory import from_numpy
from pygpukit_amd.ops._common import call, check_out, validate_float
from pygpukit_amd.ops.audio import tables
from pygpukit_amd.ops.audio.buffer import AudioBuffer

_OP_POWER, _OP_MAGNITUDE, _OP_LN, _OP_DB = 2, 3, 4, 5
_LOG_MODES = {"log10": 0, "ln": 1, None: 2}
_LAYOUTS = {"mels_first": 0, "frames_first": 1}

_windows: dict[tuple[str, int], GPUArray] = {}
_dft_tables: dict[int, GPUArray] = {}
_filterbanks: dict[tuple, "MelFilters"] = {}


class MelFilters:
    """A filterbank [n_mels, n_fft // 2 + 1] on the device with the first / last non-zero bin of each row, which the fused
    kernel's filterbank loop runs over.  Build it once (from a float array on the host or the device) and pass it as
    log_mel_features(mel_filters=...); a bare array is converted on every call."""

    def __init__(self, filters: "np.ndarray | GPUArray"):
        host = filters.astype(float32).to_numpy() if isinstance(filters, GPUArray) else filters
        host = np.ascontiguousarray(host, dtype=np.float32)
        if host.ndim != 2 or not 1 <= host.shape[0] <= tables.MAX_N_MELS:
            raise ValueError(f"mel_filters must be [n_mels <= {tables.MAX_N_MELS}, n_fft // 2 + 1], got shape {host.shape}")
        self.n_mels, self.n_freq = host.shape
        self.filters = filters if isinstance(filters, GPUArray) and filters.dtype == float32 else from_numpy(host)
        self.spans = from_numpy(tables.filter_spans(host))
        assert self.spans.dtype == int32


def _window(window, n_fft: int, name: str) -> GPUArray:
    if isinstance(window, str):
        key = (window, n_fft)
        if key not in _windows:
            _windows[key] = from_numpy(tables.window_table(window, n_fft))
        return _windows[key]
    if isinstance(window, np.ndarray):
        window = from_numpy(np.ascontiguousarray(window, dtype=np.float32))
    if not isinstance(window, GPUArray) or window.dtype != float32 or window.shape != (n_fft,):
        raise ValueError(f"{name}: window must be 'hann_periodic', 'hann' or a float32 array of {n_fft} values")
    return window


def _dft(n_fft: int) -> GPUArray:
    if n_fft not in _dft_tables:
        _dft_tables[n_fft] = from_numpy(tables.dft_table(n_fft))
    return _dft_tables[n_fft]


def _samples(audio, name: str) -> GPUArray:
    if isinstance(audio, AudioBuffer):
        audio = audio.data
    if isinstance(audio, np.ndarray):
        audio = from_numpy(np.ascontiguousarray(audio, dtype=np.float32))
    if not isinstance(audio, GPUArray) or audio.dtype != float32:
        raise ValueError(f"{name}: samples must be float32")
    return audio


def audio_log_mel_plan(n_fft: int, hop_length: int, *, stage: str = "log_mel") -> str:
    """Where the fused kernel (stage "log_mel") or stft (stage "stft") reads a workgroup's samples from: "lds" (the span of its 32
    frames is staged once) or "global" (span + window + power tile exceed the LDS budget, or PGK_AUDIO_LDS=0).  Host logic only."""
    tables.check_stft_params(int(n_fft), int(hop_length), "audio_log_mel_plan")
    if stage not in ("log_mel", "stft"):
        raise ValueError(f"audio_log_mel_plan: stage must be 'log_mel' or 'stft', got {stage!r}")
    return "lds" if _hip.load().pgk_audio_log_mel_plan(int(n_fft), int(hop_length), 1 if stage == "stft" else 0) == 1 else "global"


def log_mel_features(samples, *, n_fft: int = 400, hop_length: int = 160, window="hann_periodic", mel_filters, log="log10",
                     eps: float = 1e-10, offset: float = 0.0, scale: float = 1.0, dynamic_range: float | None = None,
                     drop_last_frame: bool = False, center: bool = True, layout: str = "mels_first",
                     dtype: "str | DataType" = float32, out: GPUArray | None = None) -> GPUArray:
    """[build-defined] samples [n] or [batch, n] (float32) -> [n_mels, n_frames] / [batch, n_mels, n_frames] (layout
    "mels_first", the Whisper encoder's) or [..., n_frames, n_mels] ("frames_first") in float32 / bfloat16 / float16.

        m = mel_filters @ |STFT(reflect-padded samples * window)|^2     n_frames = (n + 2 (n_fft // 2) - n_fft) // hop + 1
        x = log10(max(m, eps)) (log="log10"), ln(m + eps) ("ln") or m (None)
        x = max(x, x.max() - dynamic_range) over the whole call, when dynamic_range is given
        out = (x + offset) * scale, rounded once

    drop_last_frame leaves the last frame out (of the maximum too), as OpenAI's [..., :-1].  mel_filters: MelFilters or an array."""
    x = _samples(samples, "log_mel_features")
    if x.ndim not in (1, 2) or 0 in x.shape:
        raise ValueError(f"log_mel_features: samples must be [n] or [batch, n], got shape {x.shape}")
    batch, n = (1, x.shape[0]) if x.ndim == 1 else x.shape
    n_fft, hop = int(n_fft), int(hop_length)
    tables.check_stft_params(n_fft, hop, "log_mel_features")
    n_frames = tables.num_frames(n, n_fft, hop, bool(center)) - (1 if drop_last_frame else 0)
    if n_frames < 1:
        raise ValueError("log_mel_features: drop_last_frame leaves no frame")
    if log not in _LOG_MODES or layout not in _LAYOUTS:
        raise ValueError(f"log_mel_features: log must be 'log10', 'ln' or None and layout 'mels_first' or 'frames_first', got {log!r}, {layout!r}")
    if not eps > 0.0:
        raise ValueError(f"log_mel_features: eps must be positive, got {eps}")
    mf = mel_filters if isinstance(mel_filters, MelFilters) else MelFilters(mel_filters)
    if mf.n_freq != n_fft // 2 + 1:
        raise ValueError(f"log_mel_features: mel_filters has {mf.n_freq} bins, n_fft {n_fft} has {n_fft // 2 + 1}")
    if batch > 65535:
        raise ValueError(f"log_mel_features: batch {batch} > 65535")
    dt = as_dtype(dtype)
    shape = (n_frames, mf.n_mels) if _LAYOUTS[layout] else (mf.n_mels, n_frames)
    o = check_out(out, shape if x.ndim == 1 else (batch,) + shape, dt, "log_mel_features")
    validate_float(o, "log_mel_features: dtype")
    eps32 = float(np.float32(eps))
    call("pgk_audio_log_mel", x._p, _window(window, n_fft, "log_mel_features")._p, _dft(n_fft)._p, mf.filters._p, mf.spans._p, o._p,
         batch, n, n_fft, hop, 1 if center else 0, mf.n_mels, n_frames, _LOG_MODES[log], eps32, math.log10(eps32), float(offset),
         float(scale), 0 if dynamic_range is None else 1, 0.0 if dynamic_range is None else float(dynamic_range), _LAYOUTS[layout],
         dt.code, None)
    return o


def stft(audio, n_fft: int = 512, hop_length: int = 160, win_length: int = -1, center: bool = True) -> GPUArray:
    """[n] float32 -> [n_frames, n_fft // 2 + 1, 2]: [..., 0] is re, [..., 1] is im.  Periodic Hann window, reflect padding when
    centred.  win_length must be -1 or n_fft (the reference ignores it)."""
    x = _samples(audio, "stft")
    n_fft, hop = int(n_fft), int(hop_length)
    tables.check_stft_params(n_fft, hop, "stft")
    if win_length not in (-1, n_fft):
        raise ValueError(f"stft: win_length must be -1 or n_fft ({n_fft}), got {win_length}")
    if x.ndim != 1:
        raise ValueError(f"stft: samples must be 1-D, got shape {x.shape}")
    n_frames = tables.num_frames(x.size, n_fft, hop, bool(center))
    out = GPUArray((n_frames, n_fft // 2 + 1, 2), float32)
    call("pgk_audio_stft", x._p, _window("hann_periodic", n_fft, "stft")._p, _dft(n_fft)._p, out._p, x.size, n_fft, hop,
         1 if center else 0, None)
    return out


def _map(x: GPUArray, op: int, eps: float, shape, name: str) -> GPUArray:
    if x.dtype != float32:
        raise ValueError(f"{name}: input must be float32, got {x.dtype}")
    out = GPUArray(shape, float32)
    call("pgk_audio_map", x._p, out._p, out.size, op, float(eps), None)
    return out


def _stft_shape(s: GPUArray, name: str):
    if s.ndim != 3 or s.shape[2] != 2:
        raise ValueError(f"{name}: input must be [n_frames, n_freq, 2], got shape {s.shape}")
    return s.shape[:2]


def power_spectrum(stft_output: GPUArray) -> GPUArray:
    """[n_frames, n_freq, 2] -> re^2 + im^2 [n_frames, n_freq]."""
    return _map(stft_output, _OP_POWER, 0.0, _stft_shape(stft_output, "power_spectrum"), "power_spectrum")


def magnitude_spectrum(stft_output: GPUArray) -> GPUArray:
    """[n_frames, n_freq, 2] -> sqrt(re^2 + im^2) [n_frames, n_freq]."""
    return _map(stft_output, _OP_MAGNITUDE, 0.0, _stft_shape(stft_output, "magnitude_spectrum"), "magnitude_spectrum")


def create_mel_filterbank(n_mels: int = 80, n_fft: int = 512, sample_rate: int = 16000, f_min: float = 0.0, f_max: float = -1.0) -> GPUArray:
    """[n_mels, n_fft // 2 + 1] float32 (tables.mel_filterbank_htk); f_max = -1 means Nyquist."""
    if n_mels < 1 or n_fft < 2 or sample_rate < 1:
        raise ValueError(f"create_mel_filterbank: bad n_mels={n_mels} n_fft={n_fft} sample_rate={sample_rate}")
    return from_numpy(tables.mel_filterbank_htk(int(n_mels), int(n_fft), int(sample_rate), float(f_min), float(f_max)))


def apply_mel_filterbank(spectrogram: GPUArray, mel_filterbank: GPUArray) -> GPUArray:
    """[n_frames, n_freq] x [n_mels, n_freq] -> [n_frames, n_mels]: the float32 matmul_nt."""
    from pygpukit_amd.ops.matmul import matmul_nt

    if spectrogram.ndim != 2 or mel_filterbank.ndim != 2 or spectrogram.shape[1] != mel_filterbank.shape[1]:
        raise ValueError(f"apply_mel_filterbank: shapes {spectrogram.shape} and {mel_filterbank.shape} do not match")
    return matmul_nt(spectrogram, mel_filterbank)


def log_mel(mel_spectrogram: GPUArray, eps: float = 1e-10) -> GPUArray:
    """ln(x + eps)."""
    return _map(mel_spectrogram, _OP_LN, eps, mel_spectrogram.shape, "log_mel")


def to_decibels(audio, eps: float = 1e-10) -> GPUArray:
    """10 log10(x + eps)."""
    x = audio.data if isinstance(audio, AudioBuffer) else audio
    return _map(x, _OP_DB, eps, x.shape, "to_decibels")


def _htk_filters(n_mels: int, n_fft: int, sample_rate: int, f_min: float, f_max: float) -> MelFilters:
    key = (int(n_mels), int(n_fft), int(sample_rate), float(f_min), float(f_max))
    if key not in _filterbanks:
        _filterbanks[key] = MelFilters(tables.mel_filterbank_htk(*key))
    return _filterbanks[key]


def mel_spectrogram(audio, n_fft: int = 512, hop_length: int = 160, n_mels: int = 80, sample_rate: int = 16000, f_min: float = 0.0,
                    f_max: float = -1.0) -> GPUArray:
    """stft -> power -> mel filterbank as one launch of the fused kernel: [n_frames, n_mels]."""
    return log_mel_features(audio, n_fft=n_fft, hop_length=hop_length, mel_filters=_htk_filters(n_mels, n_fft, sample_rate, f_min, f_max),
                            log=None, layout="frames_first")


def log_mel_spectrogram(audio, n_fft: int = 512, hop_length: int = 160, n_mels: int = 80, sample_rate: int = 16000, f_min: float = 0.0,
                        f_max: float = -1.0, eps: float = 1e-10) -> GPUArray:
    """ln(mel_spectrogram + eps), one launch: [n_frames, n_mels]."""
    return log_mel_features(audio, n_fft=n_fft, hop_length=hop_length, mel_filters=_htk_filters(n_mels, n_fft, sample_rate, f_min, f_max),
                            log="ln", eps=eps, layout="frames_first")


__all__ = ["stft", "power_spectrum", "magnitude_spectrum", "create_mel_filterbank", "apply_mel_filterbank", "log_mel", "to_decibels",
           "mel_spectrogram", "log_mel_spectrogram", "log_mel_features", "audio_log_mel_plan", "MelFilters"]
