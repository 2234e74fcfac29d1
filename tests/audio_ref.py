"""Float64 NumPy oracle of the audio features, with the per-element error bar a float32 implementation must stay inside.

Two feature definitions:
  * "whisper": symmetric Hann window np.hanning(n_fft), reflect padding of n_fft // 2, the filterbank built from FLOORED bin
    indices up to Nyquist (whisper_filters), log10(max(m, eps)), then (x + 4) / 4;
  * "cuda": periodic Hann 0.5 (1 - cos(2 pi n / N)), HTK mel triangles evaluated at each bin's frequency in Hz with + 1e-10 in
    both denominators (htk_filters), ln(m + eps).
The window and the filterbank are INPUTS of the kernel (float32 tables), so the oracle takes them rounded to float32 and widens
them; the DFT itself is exact (np.fft.rfft in float64).

Error bar (u = 2^-24, per frame S = sum_j |x_j w_j|):
    a DFT bin is off by at most      delta = sqrt(2) (n_fft + 2) u S       (n_fft additions, the product x w, the table entry)
    its power |X|^2 by               dp = 2 |X| delta + delta^2 + 3 u |X|^2
    a mel value m by                 dm = filters @ dp + (n_freq + 1) u m
    the logarithm by                 dm / (m ln 10)   [log10; where m - dm <= eps the value must lie in the interval
                                     [log(max(m - dm, eps)), log(m + dm)] instead], plus 4 u |log| for the device function,
    then the affine map carries the interval along, and a 16-bit output adds half an ulp of its format."""

from __future__ import annotations

import numpy as np

U = 2.0 ** -24
HALF_ULP = {"float32": 0.0, "bfloat16": 2.0 ** -8, "float16": 2.0 ** -11}    # of |v|: 8 and 11 significant bits
MUTATIONS = ("window_periodic", "shift_one", "ln_for_log10", "reflect_repeats_edge", "frames_off_by_one")


def test_signal(n: int = 5280, seed: int = 12, sample_rate: int = 16000) -> np.ndarray:
    """White noise 0.05 + a 440 Hz tone 0.2 + a 3 kHz tone 0.1."""
    t = np.arange(n, dtype=np.float64) / sample_rate
    x = 0.05 * np.random.default_rng(seed).standard_normal(n) + 0.2 * np.sin(2 * np.pi * 440.0 * t) + 0.1 * np.sin(2 * np.pi * 3000.0 * t)
    return x.astype(np.float32)


test_signal.__test__ = False


def window(kind: str, n_fft: int) -> np.ndarray:
    n = np.arange(n_fft, dtype=np.float64)
    if kind == "hann":
        return (0.5 - 0.5 * np.cos(2 * np.pi * n / (n_fft - 1))).astype(np.float32)
    assert kind == "hann_periodic", kind
    return (0.5 * (1.0 - np.cos(2 * np.pi * n / n_fft))).astype(np.float32)


def whisper_filters(n_mels: int = 80, n_fft: int = 400, sample_rate: int = 16000) -> np.ndarray:
    top = 2595.0 * np.log10(1.0 + 0.5 * sample_rate / 700.0)
    edges_hz = 700.0 * (10.0 ** (np.arange(n_mels + 2) * top / (n_mels + 1) / 2595.0) - 1.0)
    edges = np.floor((n_fft + 1) * edges_hz / sample_rate).astype(np.int64)
    fb = np.zeros((n_mels, n_fft // 2 + 1))
    for i in range(n_mels):
        lo, mid, hi = edges[i:i + 3]
        for j in range(lo, mid):
            fb[i, j] = (j - lo) / (mid - lo)
        for j in range(mid, hi):
            fb[i, j] = (hi - j) / (hi - mid)
    return fb.astype(np.float32)


def htk_filters(n_mels: int, n_fft: int, sample_rate: int = 16000, f_min: float = 0.0, f_max: float = -1.0) -> np.ndarray:
    f_max = sample_rate / 2.0 if f_max < 0 else f_max
    m_lo, m_hi = (2595.0 * np.log10(1.0 + f / 700.0) for f in (f_min, f_max))
    fb = np.zeros((n_mels, n_fft // 2 + 1))
    for i in range(n_mels):
        left, mid, right = (700.0 * (10.0 ** ((m_lo + (i + d) * (m_hi - m_lo) / (n_mels + 1)) / 2595.0) - 1.0) for d in range(3))
        for j in range(n_fft // 2 + 1):
            f = j * sample_rate / n_fft
            if left <= f <= mid:
                fb[i, j] = (f - left) / (mid - left + 1e-10)
            elif mid < f <= right:
                fb[i, j] = (right - f) / (right - mid + 1e-10)
    return fb.astype(np.float32)


def n_frames(n: int, n_fft: int, hop: int, center: bool = True) -> int:
    return (n + (2 * (n_fft // 2) if center else 0) - n_fft) // hop + 1


def padded_index(n: int, n_fft: int, center: bool, length: int, repeat_edge: bool = False) -> np.ndarray:
    """Sample index of each of the first `length` positions of the (reflect-) padded signal: left src = pad - i, right
    src = n - 2 - off, both clamped to [0, n - 1]."""
    pad = n_fft // 2 if center else 0
    i = np.arange(length, dtype=np.int64)
    src = i - pad
    if repeat_edge:                                            # the mutation: ... x1 x0 | x0 x1 ...
        src = np.where(i < pad, pad - 1 - i, np.where(src >= n, 2 * n - 1 - src, src))
    else:
        src = np.where(i < pad, pad - i, np.where(src >= n, n - 2 - (src - n), src))
    return np.clip(src, 0, n - 1)


def framed(x: np.ndarray, n_fft: int, hop: int, center: bool = True, *, shift: int = 0, frames: int | None = None,
           repeat_edge: bool = False) -> np.ndarray:
    """[n_frames, n_fft] float64 frames of the padded signal."""
    x = np.asarray(x, np.float64)
    nf = n_frames(x.size, n_fft, hop, center) if frames is None else frames
    idx = padded_index(x.size, n_fft, center, (nf - 1) * hop + n_fft + shift, repeat_edge)
    return x[idx][shift + hop * np.arange(nf)[:, None] + np.arange(n_fft)[None, :]]


def stft_oracle(x, n_fft: int, hop: int, win32: np.ndarray, center: bool = True, **frame_kw):
    """(X [n_frames, n_freq] complex128, delta [n_frames, 1]): the exact DFT of the windowed frames and the bin error bar."""
    fr = framed(x, n_fft, hop, center, **frame_kw) * np.asarray(win32, np.float64)[None, :]
    delta = np.sqrt(2.0) * (n_fft + 2) * U * np.abs(fr).sum(axis=1, keepdims=True)
    return np.fft.rfft(fr, axis=1), delta


def mel_oracle(x, n_fft: int, hop: int, win32, fb32, center: bool = True, **frame_kw):
    """(m, dm) [n_frames, n_mels]: mel power and its error bar."""
    X, delta = stft_oracle(x, n_fft, hop, win32, center, **frame_kw)
    mag = np.abs(X)
    p = mag * mag
    dp = 2.0 * mag * delta + delta * delta + 3.0 * U * p
    fb = np.abs(np.asarray(fb32, np.float64))
    m = p @ np.asarray(fb32, np.float64).T
    return m, dp @ fb.T + (p.shape[1] + 1) * U * np.abs(m)


def log_interval(m, dm, log: str | None, eps: float):
    """(value, lo, hi) of the logarithm stage, the device function's 4 u |log| included."""
    if log is None:
        return m, m - dm, m + dm
    if log == "ln":
        v, lo, hi = np.log(m + eps), np.log(np.maximum(m - dm, 0.0) + eps), np.log(m + dm + eps)
    else:
        assert log == "log10", log
        v = np.log10(np.maximum(m, eps))
        live = m - dm > eps
        lin = dm / (np.where(live, m, 1.0) * np.log(10.0))
        lo = np.where(live, v - lin, np.log10(np.maximum(m - dm, eps)))
        hi = np.where(live, v + lin, np.log10(np.maximum(m + dm, eps)))
    slack = 4.0 * U * np.maximum(np.abs(lo), np.abs(hi))
    return v, lo - slack, hi + slack


def features_oracle(x, *, n_fft: int = 400, hop: int = 160, win32=None, fb32=None, log: str | None = "log10", eps: float = 1e-10,
                    offset: float = 0.0, scale: float = 1.0, center: bool = True, dynamic_range: float | None = None,
                    drop_last_frame: bool = False, layout: str = "mels_first", dtype: str = "float32", mutation: str | None = None):
    """x [n] or [batch, n] -> (value, lo, hi), each [batch, n_mels, n_frames] (or [batch, n_frames, n_mels]): what
    log_mel_features computes in exact arithmetic and the interval a float32 implementation must land in.  `mutation`: one of
    MUTATIONS, a deliberately wrong oracle for the tests of the bound itself."""
    assert mutation is None or mutation in MUTATIONS, mutation
    x = np.atleast_2d(np.asarray(x, np.float32))
    win32 = window("hann_periodic" if mutation == "window_periodic" else "hann", n_fft) if win32 is None else win32
    fb32 = whisper_filters(80, n_fft) if fb32 is None else fb32
    frames = n_frames(x.shape[1], n_fft, hop, center) - (1 if drop_last_frame else 0) + (1 if mutation == "frames_off_by_one" else 0)
    kw = dict(shift=1 if mutation == "shift_one" else 0, frames=frames, repeat_edge=mutation == "reflect_repeats_edge")
    rows = [log_interval(*mel_oracle(row, n_fft, hop, win32, fb32, center, **kw), "ln" if mutation == "ln_for_log10" else log, eps) for row in x]
    v, lo, hi = (np.stack([r[i] for r in rows]) for i in range(3))                  # [batch, n_frames, n_mels]
    if dynamic_range is not None:
        v, lo, hi = (np.maximum(a, a.max() - dynamic_range) for a in (v, lo, hi))
    v, lo, hi = ((a + offset) * scale for a in (v, lo, hi))
    if scale < 0:
        lo, hi = hi, lo
    half = HALF_ULP[dtype]
    lo, hi = lo - half * np.abs(lo) - (2.0 ** -25 if dtype == "float16" else 0.0), hi + half * np.abs(hi) + (2.0 ** -25 if dtype == "float16" else 0.0)
    if layout == "mels_first":
        v, lo, hi = (np.ascontiguousarray(a.transpose(0, 2, 1)) for a in (v, lo, hi))
    return v, lo, hi


def outside(got, lo, hi) -> np.ndarray:
    """Boolean mask of the elements outside [lo, hi]; a shape mismatch counts as everything outside."""
    got = np.asarray(got, np.float64)
    if got.shape != lo.shape:
        return np.ones(lo.shape, bool)
    return ~((got >= lo) & (got <= hi))


def used(got, v, lo, hi) -> float:
    """Largest fraction of its error bar that an element uses (1.0 = at the edge); elements with a zero-width bar count as 0 when
    exact and inf otherwise."""
    got = np.asarray(got, np.float64)
    err, room = np.abs(got - v), np.maximum(np.maximum(hi - v, v - lo), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(room > 0, err / room, np.where(err == 0, 0.0, np.inf))
    return float(frac.max())


def float32_pipeline(x, *, n_fft: int = 400, hop: int = 160, win32=None, fb32=None, eps: float = 1e-10, center: bool = True) -> np.ndarray:
    """The whisper definition computed the way a float32 device computes it: float32 window product, float32 cos / -sin tables,
    float32 matrix products, float32 log10 and affine.  [1, n_mels, n_frames]."""
    win32 = window("hann", n_fft) if win32 is None else win32
    fb32 = whisper_filters(80, n_fft) if fb32 is None else fb32
    fr = (framed(x, n_fft, hop, center).astype(np.float32) * win32[None, :]).astype(np.float32)
    ang = 2 * np.pi * ((np.arange(n_fft)[:, None] * np.arange(n_fft // 2 + 1)[None, :]) % n_fft) / n_fft
    re, im = fr @ np.cos(ang).astype(np.float32), fr @ (-np.sin(ang)).astype(np.float32)
    m = (re * re + im * im).astype(np.float32) @ fb32.T
    out = (np.log10(np.maximum(m, np.float32(eps))).astype(np.float32) + np.float32(4.0)) * np.float32(0.25)
    return np.ascontiguousarray(out.T)[None]


def bf16_to_f32(bits: np.ndarray) -> np.ndarray:
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def resample_oracle(x, taps32: np.ndarray | None, src: int, dst: int):
    """(value, bound) of ops.audio.resample in float64.  Decimator: out[i] = sum_t taps[t] x[i ratio - n_taps / 2 + t] within
    n_taps u sum |x h|; linear: x[p] + frac (x[p + 1] - x[p]) at p = i src // dst, frac = (i src % dst) / dst, within
    4 u (|x[p]| + |x[p + 1]|) (the fraction, the difference, the product and the sum are each rounded once)."""
    x = np.asarray(x, np.float64)
    n, n_out = x.size, x.size * dst // src
    i = np.arange(n_out, dtype=np.int64)
    if src == dst:
        return x.copy(), np.zeros(n)
    if taps32 is not None:
        h, ratio = np.asarray(taps32, np.float64), src // dst
        idx = i[:, None] * ratio - h.size // 2 + np.arange(h.size)[None, :]
        terms = np.where((idx >= 0) & (idx < n), x[np.clip(idx, 0, n - 1)], 0.0) * h[None, :]
        return terms.sum(axis=1), h.size * U * np.abs(terms).sum(axis=1)
    p, frac = i * src // dst, ((i * src) % dst) / dst
    s0 = x[np.minimum(p, n - 1)]
    s1 = np.where(p + 1 < n, x[np.minimum(p + 1, n - 1)], s0)
    return s0 + frac * (s1 - s0), 4.0 * U * (np.abs(s0) + np.abs(s1))
