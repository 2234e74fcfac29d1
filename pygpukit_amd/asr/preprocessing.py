"""Whisper audio preprocessing (reference: src/pygpukit/asr/preprocessing.py, which cannot run: its radix-2 stft refuses n_fft =
400; and WhisperModel._compute_mel_numpy, the path that does run, on the host).

preprocess_audio is ONE launch of the fused log-mel kernel (ops.audio.log_mel_features) on the device, after pad_or_trim (a memset
and a device copy).  The feature definition is that of the reference's runnable path:
    symmetric Hann window np.hanning(400), reflect padding of 200, hop 160 -> 3001 frames for 30 s,
    filterbank from floored bin indices up to Nyquist (whisper_mel_filters; four of its 80 rows are empty),
    log10(max(mel, 1e-10)), then (x + 4) / 4.
The keywords window=, mel_filters=, dynamic_range=, drop_last_frame= and dtype= reach the kernel, so a caller holding OpenAI's
filter file gets OpenAI's features: window="hann_periodic", mel_filters=<file>, dynamic_range=8.0, drop_last_frame=True."""

from __future__ import annotations

import numpy as np

from pygpukit_amd import _hip
from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import DataType, float32
from pygpukit_amd.core.factory import from_numpy
from pygpukit_amd.ops import audio
from pygpukit_amd.ops.audio.spectral import MelFilters

WHISPER_SAMPLE_RATE = 16000
WHISPER_N_FFT = 400
WHISPER_HOP_LENGTH = 160
WHISPER_N_MELS = 80
WHISPER_CHUNK_LENGTH = 30  # seconds
WHISPER_N_SAMPLES = WHISPER_SAMPLE_RATE * WHISPER_CHUNK_LENGTH  # 480000
WHISPER_N_FRAMES = WHISPER_N_SAMPLES // WHISPER_HOP_LENGTH  # 3000

_filters: dict[tuple[int, int, int], MelFilters] = {}


def whisper_mel_filters(n_mels: int = WHISPER_N_MELS, n_fft: int = WHISPER_N_FFT, sample_rate: int = WHISPER_SAMPLE_RATE) -> np.ndarray:
    """[n_mels, n_fft // 2 + 1] float64: n_mels + 2 points equally spaced on the HTK mel scale from 0 to Nyquist, converted to bin
    indices floor((n_fft + 1) * hz / sample_rate); row i rises (j - left) / (center - left) over [left, center) and falls
    (right - j) / (right - center) over [center, right).  Rows whose three indices coincide are empty."""
    mel_max = 2595.0 * np.log10(1.0 + (sample_rate / 2.0) / 700.0)
    hz = 700.0 * (10.0 ** (np.linspace(0.0, mel_max, n_mels + 2) / 2595.0) - 1.0)
    bins = np.floor((n_fft + 1) * hz / sample_rate).astype(int)
    fb = np.zeros((n_mels, n_fft // 2 + 1))
    for i in range(n_mels):
        left, center, right = bins[i], bins[i + 1], bins[i + 2]
        j = np.arange(left, center)
        fb[i, j] = (j - left) / max(center - left, 1)
        j = np.arange(center, right)
        fb[i, j] = (right - j) / max(right - center, 1)
    return fb


def _whisper_filters(n_mels: int) -> MelFilters:
    key = (int(n_mels), WHISPER_N_FFT, WHISPER_SAMPLE_RATE)
    if key not in _filters:
        _filters[key] = MelFilters(whisper_mel_filters(*key))
    return _filters[key]


def _to_device(audio_data) -> GPUArray:
    if isinstance(audio_data, audio.AudioBuffer):
        audio_data = audio_data.data
    if isinstance(audio_data, np.ndarray):
        audio_data = from_numpy(np.ascontiguousarray(audio_data, dtype=np.float32))
    if not isinstance(audio_data, GPUArray):
        raise TypeError(f"Unsupported audio input type: {type(audio_data)}")
    if audio_data.dtype != float32 or audio_data.ndim != 1:
        raise ValueError(f"audio must be 1-D float32 samples, got {audio_data.dtype} of shape {audio_data.shape}")
    return audio_data


def _copy_into(dst: GPUArray, dst_offset: int, src: GPUArray, count: int) -> None:
    if count:
        _hip.call("pgk_memcpy_d2d", _hip.C.c_void_p(dst._ptr + 4 * dst_offset), src._p, 4 * count, None)


def pad_or_trim(audio_data, length: int = WHISPER_N_SAMPLES) -> GPUArray:
    """Exactly `length` samples: trimmed, or zero-padded at the end.  On the device: a memset and a copy, no host concatenate.
    An input of the right length is returned as it is."""
    x = _to_device(audio_data)
    if x.size == length:
        return x
    out = GPUArray((int(length),), float32)
    if x.size < length:
        out.fill_zeros()
    _copy_into(out, 0, x, min(x.size, int(length)))
    return out


def normalize_mel(log_mel) -> GPUArray:
    """(log_mel + 4) / 4 as an op of its own (preprocess_audio fuses it into the kernel's epilogue)."""
    if isinstance(log_mel, np.ndarray):
        log_mel = from_numpy(np.ascontiguousarray(log_mel, dtype=np.float32))
    return (log_mel + 4.0) / 4.0


def load_audio(path: str) -> "tuple[np.ndarray, int]":
    """A file -> (mono float32 samples, sample rate).  Needs soundfile."""
    try:
        import soundfile as sf
    except ImportError as err:
        raise ImportError("soundfile is required to load audio files. Install with: pip install soundfile") from err
    data, rate = sf.read(path)
    if data.ndim > 1:
        data = data.mean(axis=1)
    return data.astype(np.float32), int(rate)


def _prepare(audio_input, sample_rate, padding: bool) -> GPUArray:
    if isinstance(audio_input, str):
        audio_input, sample_rate = load_audio(audio_input)
    x = _to_device(audio_input)
    rate = int(sample_rate or WHISPER_SAMPLE_RATE)
    if rate != WHISPER_SAMPLE_RATE:
        x = audio.resample(x, rate, WHISPER_SAMPLE_RATE)
    return pad_or_trim(x, WHISPER_N_SAMPLES) if padding else x


def _features(samples: GPUArray, n_mels: int, window, mel_filters, dynamic_range, drop_last_frame: bool, dtype) -> GPUArray:
    return audio.log_mel_features(samples, n_fft=WHISPER_N_FFT, hop_length=WHISPER_HOP_LENGTH, window=window,
                                  mel_filters=_whisper_filters(n_mels) if mel_filters is None else mel_filters, log="log10", eps=1e-10,
                                  offset=4.0, scale=0.25, dynamic_range=dynamic_range, drop_last_frame=drop_last_frame, dtype=dtype)


def preprocess_audio(audio_input, sample_rate: int | None = None, n_mels: int = WHISPER_N_MELS, padding: bool = True, *, window="hann",
                     mel_filters=None, dynamic_range: float | None = None, drop_last_frame: bool = False,
                     dtype: "str | DataType" = float32) -> GPUArray:
    """Samples (GPUArray / ndarray / AudioBuffer, or a file path when soundfile is installed) -> normalised log-mel
    [n_mels, n_frames] in `dtype`: [80, 3001] for the padded 30 s.  sample_rate other than 16000 goes through ops.audio.resample."""
    return _features(_prepare(audio_input, sample_rate, padding), n_mels, window, mel_filters, dynamic_range, drop_last_frame, dtype)


def preprocess_audio_batch(audio_list: list, sample_rate: int | None = None, n_mels: int = WHISPER_N_MELS, *, window="hann", mel_filters=None,
                           dynamic_range: float | None = None, drop_last_frame: bool = False, dtype: "str | DataType" = float32) -> GPUArray:
    """[batch, n_mels, n_frames]: every item padded to 30 s into one [batch, 480000] buffer, then ONE launch for the batch.
    dynamic_range then takes its maximum over the whole batch."""
    if not audio_list:
        raise ValueError("preprocess_audio_batch: empty list")
    rows = GPUArray((len(audio_list), WHISPER_N_SAMPLES), float32)
    rows.fill_zeros()
    for i, item in enumerate(audio_list):
        x = _prepare(item, sample_rate, False)
        _copy_into(rows, i * WHISPER_N_SAMPLES, x, min(x.size, WHISPER_N_SAMPLES))
    return _features(rows, n_mels, window, mel_filters, dynamic_range, drop_last_frame, dtype)


__all__ = ["preprocess_audio", "preprocess_audio_batch", "pad_or_trim", "normalize_mel", "whisper_mel_filters", "load_audio",
           "WHISPER_SAMPLE_RATE", "WHISPER_N_FFT", "WHISPER_HOP_LENGTH", "WHISPER_N_MELS", "WHISPER_CHUNK_LENGTH", "WHISPER_N_SAMPLES",
           "WHISPER_N_FRAMES"]
