"""Host arithmetic of ops.audio: windows, the DFT table, mel filterbanks and the decimator's taps, all in float64 and rounded
once to float32.  Pure NumPy, needs no device; the device copies are cached per parameter set in spectral.py / buffer.py, as the
RoPE tables are."""

from __future__ import annotations

import numpy as np

MIN_N_FFT, MAX_N_FFT, MAX_N_MELS = 16, 2048, 256


def check_stft_params(n_fft: int, hop_length: int, name: str) -> None:
    if n_fft % 2 or not MIN_N_FFT <= n_fft <= MAX_N_FFT:
        raise ValueError(f"{name}: n_fft must be even and in [{MIN_N_FFT}, {MAX_N_FFT}], got {n_fft}")
    if not 1 <= hop_length <= n_fft:
        raise ValueError(f"{name}: hop_length must be in [1, n_fft], got {hop_length} for n_fft {n_fft}")


def num_frames(n: int, n_fft: int, hop_length: int, center: bool = True) -> int:
    """(n + 2 * (n_fft // 2) - n_fft) // hop + 1 when centred; (n - n_fft) // hop + 1 otherwise (needs n >= n_fft)."""
    padded = n + (2 * (n_fft // 2) if center else 0)
    if n < 1 or padded < n_fft:
        raise ValueError(f"stft: {n} samples are too short for n_fft {n_fft} (center={center})")
    return (padded - n_fft) // hop_length + 1


def window_table(kind: str, n_fft: int) -> np.ndarray:
    """"hann_periodic": 0.5 (1 - cos(2 pi n / N)), the reference's CUDA window; "hann": symmetric, np.hanning(N)."""
    n = np.arange(n_fft, dtype=np.float64)
    if kind == "hann_periodic":
        w = 0.5 * (1.0 - np.cos(2.0 * np.pi * n / n_fft))
    elif kind == "hann":
        w = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / (n_fft - 1))
    else:
        raise ValueError(f"window must be 'hann_periodic', 'hann' or an array of n_fft values, got {kind!r}")
    return w.astype(np.float32)


def padded_bins(n_fft: int) -> int:
    return -(-(n_fft // 2 + 1) // 32) * 32


def dft_table(n_fft: int) -> np.ndarray:
    """[2, n_fft, padded_bins] float32: cos(2 pi k bin / n_fft) and -sin(...), zeros in the padding.  The angle is reduced in
    integers (k * bin mod n_fft) before it meets a float."""
    n_freq, nbp = n_fft // 2 + 1, padded_bins(n_fft)
    k = np.arange(n_fft, dtype=np.int64)[:, None]
    b = np.arange(n_freq, dtype=np.int64)[None, :]
    ang = 2.0 * np.pi * ((k * b) % n_fft).astype(np.float64) / n_fft
    t = np.zeros((2, n_fft, nbp), np.float32)
    t[0, :, :n_freq] = np.cos(ang)
    t[1, :, :n_freq] = -np.sin(ang)
    return t


def mel_filterbank_htk(n_mels: int, n_fft: int, sample_rate: int, f_min: float = 0.0, f_max: float = -1.0) -> np.ndarray:
    """The reference's CUDA filterbank: HTK mel scale 2595 log10(1 + f / 700), n_mels + 2 points equally spaced in mel, triangles
    evaluated at each bin's frequency in Hz with + 1e-10 in both denominators.  f_max < 0: Nyquist."""
    if f_max < 0:
        f_max = sample_rate / 2.0
    mel = lambda hz: 2595.0 * np.log10(1.0 + hz / 700.0)               # noqa: E731
    pts = mel(f_min) + (mel(f_max) - mel(f_min)) / (n_mels + 1) * np.arange(n_mels + 2, dtype=np.float64)
    hz = 700.0 * (10.0 ** (pts / 2595.0) - 1.0)
    left, center, right = hz[:-2, None], hz[1:-1, None], hz[2:, None]
    f = np.arange(n_fft // 2 + 1, dtype=np.float64)[None, :] * sample_rate / n_fft
    rise = (f - left) / (center - left + 1e-10)
    fall = (right - f) / (right - center + 1e-10)
    fb = np.where((f >= left) & (f <= center), rise, np.where((f > center) & (f <= right), fall, 0.0))
    return fb.astype(np.float32)


def filter_spans(fb: np.ndarray) -> np.ndarray:
    """[n_mels, 2] int32: first and last non-zero bin of each row (inclusive); (0, -1) for an empty row."""
    spans = np.empty((fb.shape[0], 2), np.int32)
    for m, row in enumerate(fb):
        nz = np.flatnonzero(row)
        spans[m] = (nz[0], nz[-1]) if nz.size else (0, -1)
    return spans


def decimator_taps(ratio: int) -> np.ndarray:
    """Kaiser windowed-sinc low-pass for src = ratio * dst: cutoff 0.45 * dst, beta 5, unit DC gain, 2 * ceil(16 * ratio / 3)
    taps (32 at ratio 3).  Tap t multiplies x[i * ratio - n_taps / 2 + t], so the filter is centred on tap n_taps / 2."""
    if ratio < 2:
        raise ValueError(f"decimator_taps: ratio must be >= 2, got {ratio}")
    half = -(-16 * ratio // 3)
    tau = np.arange(-half, half, dtype=np.float64)
    fc = 0.45 / ratio                                                   # cycles per input sample
    h = 2.0 * fc * np.sinc(2.0 * fc * tau) * np.i0(5.0 * np.sqrt(np.maximum(0.0, 1.0 - (tau / half) ** 2))) / np.i0(5.0)
    return (h / h.sum()).astype(np.float32)


def resampled_length(n: int, src: int, dst: int) -> int:
    return n * dst // src
