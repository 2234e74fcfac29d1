"""ops.audio on the GPU against the float64 oracle and its derived error bar (tests/audio_ref.py): every element of every case
must lie inside its own interval.  Shapes sit where the fused kernel can go wrong: one partial 32-frame tile (11 frames), a full
tile + the boundary + a tile of two (34 frames), a signal shorter than the padding (the reflect clamp is live), no centring, tiny
and non-power-of-two n_fft (16, 18: the k loop's remainder), n_fft 512, 128 mels, hop = n_fft, batch 2, both layouts, three output
dtypes, both log modes, and both sample paths (LDS span / global reads: n_fft 2048, and PGK_AUDIO_LDS=0 at the Whisper shape).

Measured on an MI355X (each test prints its figure): float32 outputs use at most 2 % of their bar at the Whisper shape and 11 % at
n_fft 16 / hop 1; ln mode 58 % (the empty rows, whose bar is the 4 u |log| of the device function alone); 16-bit outputs up to 92 %
(their bar is dominated by the half ulp of the format)."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from tests import audio_ref as R
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu


def _host(a, dtype: str = "float32") -> np.ndarray:
    h = a.to_numpy()
    return R.bf16_to_f32(h) if dtype == "bfloat16" else h.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _filters(kind: str, n_mels: int, n_fft: int) -> np.ndarray:
    if kind == "whisper":
        return R.whisper_filters(n_mels, n_fft)
    if kind == "eye":
        return np.eye(n_fft // 2 + 1, dtype=np.float32)
    return R.htk_filters(n_mels, n_fft)


def _run(x, *, n_fft=400, hop=160, window="hann", filters=("whisper", 80), log="log10", offset=4.0, scale=0.25, center=True,
         dynamic_range=None, drop_last_frame=False, layout="mels_first", dtype="float32", eps=1e-10):
    """(gpu result as float32, oracle value, lo, hi), all [batch, ...]."""
    from pygpukit_amd.core.factory import from_numpy
    from pygpukit_amd.ops import audio

    fb = _filters(filters[0], filters[1], n_fft)
    got = audio.log_mel_features(from_numpy(np.ascontiguousarray(x, np.float32)), n_fft=n_fft, hop_length=hop, window=window, mel_filters=fb,
                                 log=log, eps=eps, offset=offset, scale=scale, center=center, dynamic_range=dynamic_range,
                                 drop_last_frame=drop_last_frame, layout=layout, dtype=dtype)
    v, lo, hi = R.features_oracle(x, n_fft=n_fft, hop=hop, win32=R.window(window, n_fft), fb32=fb, log=log, eps=eps, offset=offset, scale=scale,
                                  center=center, dynamic_range=dynamic_range, drop_last_frame=drop_last_frame, layout=layout, dtype=dtype)
    got = _host(got, dtype)
    return (got[None] if np.ndim(x) == 1 else got), v, lo, hi


def _check(what: str, got, v, lo, hi) -> None:
    assert got.shape == v.shape, (what, got.shape, v.shape)
    bad = R.outside(got, lo, hi)
    print(f"{what}: shape {got.shape}, outside {int(bad.sum())} of {bad.size}, largest share of the bar used {R.used(got, v, lo, hi):.3g}")
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5])


CASES = {
    "11_frames": dict(n=1600), "34_frames": dict(n=5280), "shorter_than_pad": dict(n=150), "one_sample": dict(n=1),
    "uncentred": dict(n=1600, center=False), "nfft16_hop4_5mels": dict(n=203, n_fft=16, hop=4, filters=("htk", 5), window="hann_periodic"),
    "nfft18_hop5_3mels": dict(n=333, n_fft=18, hop=5, filters=("htk", 3)), "nfft512": dict(n=1600, n_fft=512, filters=("htk", 80)),
    "128_mels": dict(n=1600, filters=("htk", 128)), "hop_is_nfft": dict(n=5280, hop=400), "hop_1": dict(n=100, n_fft=16, hop=1, filters=("htk", 4)),
    "global_nfft2048": dict(n=40000, n_fft=2048, hop=512, filters=("htk", 8)), "256_mels": dict(n=1600, n_fft=512, filters=("htk", 256)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_features_within_the_bar(name):
    from pygpukit_amd.ops import audio

    kw = dict(CASES[name])
    x = R.test_signal(kw.pop("n"))
    assert audio.audio_log_mel_plan(kw.get("n_fft", 400), kw.get("hop", 160)) == ("global" if name.startswith("global") else "lds")
    _check(name, *_run(x, **kw))


@pytest.mark.parametrize("layout", ["mels_first", "frames_first"])
@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("log", ["log10", "ln"])
def test_layouts_dtypes_and_log_modes_batch_2(layout, dtype, log):
    sig = R.test_signal(5280)
    x = np.stack([sig[:2000], 2.5 * sig[3000:5000][::-1]])                       # different contents per row
    _check(f"{layout} {dtype} {log}", *_run(x, layout=layout, dtype=dtype, log=log))


def test_global_sample_path_at_the_whisper_shape(monkeypatch):
    from pygpukit_amd.ops import audio

    x = np.stack([R.test_signal(5280), R.test_signal(5280, seed=13)])
    lds = _run(x)
    monkeypatch.setenv("PGK_AUDIO_LDS", "0")
    assert audio.audio_log_mel_plan(400, 160) == "global"
    glob = _run(x)
    _check("global path", *glob)
    assert np.array_equal(lds[0], glob[0])                                       # same arithmetic, only the sample source differs


def test_silence_and_empty_rows_are_exact():
    got = _run(np.zeros((2, 1600), np.float32))[0]
    assert (got == -1.5).all()                                                   # (log10(1e-10) + 4) / 4
    for dtype in ("float32", "bfloat16", "float16"):
        got = _run(R.test_signal(5280), dtype=dtype)[0]
        empty = _filters("whisper", 80, 400).sum(axis=1) == 0
        assert int(empty.sum()) == 4 and (got[0][empty] == -1.5).all() and (got[0][~empty] != -1.5).any()


@pytest.mark.parametrize("p", [0, 1599, 777])
def test_unit_impulse_fixes_frame_alignment(p):
    """A unit impulse at sample p (one that the reflection does not duplicate): every frame that contains it has the power
    w[p + pad - start]^2 in EVERY bin; every other frame is silent."""
    n, n_fft, hop = 1600, 400, 160
    x = np.zeros(n, np.float32)
    x[p] = 1.0
    got, v, lo, hi = _run(x, filters=("eye", 201), log=None, offset=0.0, scale=1.0, layout="frames_first")
    w = R.window("hann", n_fft).astype(np.float64)
    want = np.zeros((11, 201))
    for f in range(11):
        k = p + n_fft // 2 - f * hop
        if 0 <= k < n_fft:
            want[f, :] = w[k] ** 2
    assert np.abs(v[0] - want).max() < 1e-12
    _check(f"impulse at {p}", got, v, lo, hi)
    assert (got[0][want == 0] == 0.0).all()


def test_impulses_near_the_edges_are_reflected():
    x = np.zeros(1600, np.float32)
    x[3], x[1595] = 1.0, -0.5                                                    # each appears twice in the padded signal
    _check("reflected impulses", *_run(x, filters=("eye", 201), log=None, offset=0.0, scale=1.0))


def test_cosine_on_an_integer_bin():
    n_fft, b = 400, 37
    x = (0.5 * np.cos(2 * np.pi * b * np.arange(1600) / n_fft)).astype(np.float32)
    got, v, lo, hi = _run(x, window="hann_periodic", filters=("eye", 201), log=None, offset=0.0, scale=1.0, center=False, layout="frames_first")
    _check("cosine", got, v, lo, hi)
    far = np.ones(201, bool)
    far[b - 1:b + 2] = False                                                     # the Hann main lobe: b and its neighbours
    assert (got[0].argmax(axis=1) == b).all() and got[0][:, far].max() < 1e-9 * got[0][:, b].min()
    assert np.allclose(got[0][:, b], (0.5 * n_fft / 4) ** 2, rtol=1e-4)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("drop", [False, True])
def test_dynamic_range_with_the_maximum_in_the_last_partial_tile(dtype, drop):
    sig = R.test_signal(5280)
    x = np.stack([0.01 * sig, 0.01 * sig[::-1]])
    x[1, -60:] += 0.9                                                            # loudest in frame 33 of row 1: the tile of two
    got, v, lo, hi = _run(x, dynamic_range=3.0, drop_last_frame=drop, dtype=dtype)
    full = R.features_oracle(x, offset=4.0, scale=0.25)[0]
    assert np.unravel_index(full.argmax(), full.shape)[0::2] == (1, 33)
    assert got.shape == (2, 80, 33 if drop else 34) and (v == v.min()).mean() > 0.2          # the clamp is live
    _check(f"dynamic_range {dtype} drop={drop}", got, v, lo, hi)
    if not drop:
        assert got.min() == pytest.approx(got.max() - 0.75, abs=1e-2)


def test_parameter_checks():
    from pygpukit_amd.core.factory import from_numpy
    from pygpukit_amd.ops import audio

    x = from_numpy(R.test_signal(300))
    fb = _filters("whisper", 80, 400)
    for kw in (dict(n_fft=402), dict(n_fft=14), dict(hop_length=401), dict(log="log2"), dict(layout="x"), dict(center=False), dict(dtype="int32"),
               dict(eps=0.0), dict(n_fft=512)):
        with pytest.raises(ValueError):
            audio.log_mel_features(x, mel_filters=fb, **kw)
    with pytest.raises(ValueError):
        audio.stft(x, n_fft=400, win_length=200)
    assert audio.stft(x, n_fft=400, win_length=400).shape == (2, 201, 2)


# ------------------------------------------------------------------------------------------------ the unfused ops
@pytest.mark.parametrize("n, n_fft, hop, center", [(5280, 400, 160, True), (1600, 512, 160, True), (150, 400, 160, True), (1600, 400, 400, False),
                                                    (40000, 2048, 2048, True), (333, 18, 5, True)])
def test_unfused_chain_stage_by_stage(n, n_fft, hop, center):
    from pygpukit_amd.core.factory import from_numpy
    from pygpukit_amd.ops import audio

    x = R.test_signal(n)
    win, fb = R.window("hann_periodic", n_fft), R.htk_filters(40, n_fft)
    X, delta = R.stft_oracle(x, n_fft, hop, win, center)
    s = audio.stft(from_numpy(x), n_fft=n_fft, hop_length=hop, center=center)
    sh = s.to_numpy()
    assert sh.shape == X.shape + (2,)
    assert (np.abs(sh[..., 0] - X.real) <= delta).all() and (np.abs(sh[..., 1] - X.imag) <= delta).all()      # [..., 0] re, [..., 1] im
    mag = np.abs(X)
    dp = 2 * mag * delta + delta ** 2 + 3 * R.U * mag ** 2
    p = audio.power_spectrum(s)
    assert p.shape == X.shape and (np.abs(p.to_numpy() - mag ** 2) <= dp).all()
    with np.errstate(divide="ignore", invalid="ignore"):
        dmag = np.where(mag > delta, dp / np.maximum(mag, 1e-300) + R.U * mag, np.sqrt(dp) + R.U * mag)
    assert (np.abs(audio.magnitude_spectrum(s).to_numpy() - mag) <= dmag).all()
    m, dm = R.mel_oracle(x, n_fft, hop, win, fb, center)
    mel = audio.apply_mel_filterbank(p, audio.create_mel_filterbank(40, n_fft))
    assert mel.shape == m.shape and (np.abs(mel.to_numpy() - m) <= dm).all()
    mel64 = mel.to_numpy().astype(np.float64)
    ln = np.log(mel64 + 1e-10)
    assert (np.abs(audio.log_mel(mel).to_numpy() - ln) <= 4 * R.U * np.abs(ln) + 2 * R.U).all()
    db = 10 * np.log10(mel64 + 1e-10)
    assert (np.abs(audio.to_decibels(mel).to_numpy() - db) <= 6 * R.U * np.abs(db) + 2 * R.U).all()
    for fused, log in ((audio.mel_spectrogram, None), (audio.log_mel_spectrogram, "ln")):
        got = fused(from_numpy(x), n_fft=n_fft, hop_length=hop, n_mels=40) if center else None
        if got is not None:
            v, lo, hi = R.features_oracle(x, n_fft=n_fft, hop=hop, win32=win, fb32=fb, log=log, layout="frames_first")
            _check(f"{fused.__name__} n_fft {n_fft}", got.to_numpy()[None], v, lo, hi)


@pytest.mark.parametrize("n", [1, 255, 257, 4099])
def test_pcm_and_mono_are_bit_exact(n):
    from pygpukit_amd.core.factory import from_numpy
    from pygpukit_amd.ops import audio

    rng = np.random.default_rng(n)
    pcm = rng.integers(-32768, 32768, n, dtype=np.int16)
    pcm[0] = -32768
    assert np.array_equal(audio.pcm_to_float32(from_numpy(pcm)).to_numpy(), pcm.astype(np.float32) / np.float32(32768.0))
    st = rng.standard_normal(2 * n).astype(np.float32)
    assert np.array_equal(audio.stereo_to_mono(from_numpy(st)).to_numpy(), (st[0::2] + st[1::2]) * np.float32(0.5))
    buf = audio.from_pcm(rng.integers(-32768, 32768, 2 * n, dtype=np.int16), sample_rate=48000, channels=2).to_mono()
    assert buf.channels == 1 and buf.data.shape == (n,) and buf.sample_rate == 48000 and buf.to_numpy().dtype == np.float32


@pytest.mark.parametrize("n", [1, 1023, 1025, 48001])
def test_normalize_peak_and_rms(n):
    from pygpukit_amd.core.factory import from_numpy
    from pygpukit_amd.ops import audio

    x = (0.3 * np.random.default_rng(n).standard_normal(n)).astype(np.float32)
    x64 = x.astype(np.float64)
    a = from_numpy(x)
    audio.normalize_peak(a)
    scale = np.float32(1.0) / np.abs(x).max()
    assert np.array_equal(a.to_numpy(), x * scale)
    buf = audio.AudioBuffer(from_numpy(x), 16000, 1).normalize("rms", target_db=-20.0)
    want = x64 * (10 ** (-20.0 / 20) / np.sqrt(np.mean(x64 ** 2)))
    assert (np.abs(buf.to_numpy() - want) <= 3 * R.U * np.abs(want)).all()
    z = from_numpy(np.zeros(n, np.float32))
    audio.normalize_peak(z)
    audio.normalize_rms(z)
    assert not z.to_numpy().any()


@pytest.mark.parametrize("src, dst, n", [(48000, 16000, 4801), (48000, 16000, 31), (32000, 16000, 3001), (44100, 16000, 4411), (16000, 16000, 777),
                                         (16000, 48000, 100), (96000, 16000, 5003)])
def test_resample_against_the_same_taps(src, dst, n):
    from pygpukit_amd.core.factory import from_numpy
    from pygpukit_amd.ops import audio

    x = R.test_signal(n, sample_rate=src)
    taps = audio.tables.decimator_taps(src // dst) if src % dst == 0 and src != dst else None
    v, bound = R.resample_oracle(x, taps, src, dst)
    got = audio.resample(from_numpy(x), src, dst).to_numpy()
    assert got.shape == (n * dst // src,) == v.shape
    assert (np.abs(got - v) <= bound).all()


@pytest.mark.parametrize("freq", [1000.0, 10000.0])
def test_resampled_tone_has_the_taps_own_gain(freq):
    """48 k -> 16 k: a tone comes out with amplitude |H(f)| of the taps (10 kHz aliases to 6 kHz at that amplitude)."""
    from pygpukit_amd.core.factory import from_numpy
    from pygpukit_amd.ops import audio

    n = 9600
    x = np.sin(2 * np.pi * freq * np.arange(n) / 48000.0).astype(np.float32)
    y = audio.AudioBuffer(from_numpy(x), 48000, 1).resample(16000).to_numpy().astype(np.float64)[16:-16]      # clear of the zero edges
    h = audio.tables.decimator_taps(3).astype(np.float64)
    gain = abs(np.exp(-2j * np.pi * freq / 48000.0 * np.arange(h.size)) @ h)
    t = np.arange(16, 16 + y.size) / 16000.0
    basis = np.stack([np.sin(2 * np.pi * freq * t), np.cos(2 * np.pi * freq * t)], axis=1)
    coef = np.linalg.lstsq(basis, y, rcond=None)[0]
    print(f"{freq} Hz: |H| {gain:.6f}, fitted amplitude {np.hypot(*coef):.6f}")
    assert abs(np.hypot(*coef) - gain) < 1e-5 and (gain > 0.99 if freq == 1000.0 else gain < 0.02)


# ------------------------------------------------------------------------------------------------ asr.preprocessing
def test_preprocess_audio_against_the_oracle_and_the_record():
    from pygpukit_amd.asr import preprocessing as P
    from pygpukit_amd.core.factory import from_numpy

    g = load_golden("g12_whisper_mel.npz")
    short = g["short"]
    mel = P.preprocess_audio(short)
    assert mel.shape == (80, 3001)
    x = np.zeros(480000, np.float32)
    x[:1600] = short
    v, lo, hi = R.features_oracle(x, offset=4.0, scale=0.25)
    got = mel.to_numpy()
    _check("preprocess_audio 30 s", got[None], v, lo, hi)
    # the record (a complex64 computation on the host) sits in the same intervals (test_audio_cpu.py), so the two differ by less than their width
    assert (np.abs(got[:, :40] - g["first"]) <= (hi - lo)[0, :, :40] + 2.0 ** -21).all() and np.array_equal(got[:, -8:], g["last"])
    assert np.array_equal(P.preprocess_audio(from_numpy(short)).to_numpy(), got)
    unpadded = P.preprocess_audio(short, padding=False)
    assert unpadded.shape == (80, 11)
    bf = P.preprocess_audio(short, dtype="bfloat16")
    vb, lob, hib = R.features_oracle(x, offset=4.0, scale=0.25, dtype="bfloat16")
    _check("preprocess_audio bf16", _host(bf, "bfloat16")[None], vb, lob, hib)
    openai = P.preprocess_audio(short, window="hann_periodic", dynamic_range=8.0, drop_last_frame=True)
    vo, loo, hio = R.features_oracle(x, win32=R.window("hann_periodic", 400), offset=4.0, scale=0.25, dynamic_range=8.0, drop_last_frame=True)
    assert openai.shape == (80, 3000)
    _check("OpenAI's variant", openai.to_numpy()[None], vo, loo, hio)


def test_preprocess_batch_pad_or_trim_and_normalize_mel():
    from pygpukit_amd.asr import preprocessing as P

    g = load_golden("g12_whisper_mel.npz")
    short, signal = g["short"], g["signal"]
    batch = P.preprocess_audio_batch([short, signal])
    assert batch.shape == (2, 80, 3001)
    assert np.array_equal(batch.to_numpy()[0], P.preprocess_audio(short).to_numpy()) and np.array_equal(batch.to_numpy()[1], P.preprocess_audio(signal).to_numpy())
    assert P.pad_or_trim(short, 1000).shape == (int(g["trimmed_len"]),) and np.array_equal(P.pad_or_trim(short, 1000).to_numpy(), short[:1000])
    padded = P.pad_or_trim(short, 2000).to_numpy()
    assert padded.shape == (2000,) and np.array_equal(padded[:1600], short) and np.array_equal(padded[-400:], g["padded_tail"])
    assert P.pad_or_trim(short, 1600).to_numpy().shape == (1600,)
    assert np.allclose(P.normalize_mel(g["mel"].astype(np.float32)).to_numpy(), g["normalized"], atol=1e-6)
    up = P.preprocess_audio(np.repeat(short, 3), sample_rate=48000, padding=False)
    assert up.shape == (80, 11)
