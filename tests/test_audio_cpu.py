"""ops.audio and asr.preprocessing without a device: the oracle (tests/audio_ref.py) against the fixture recorded from the
reference, the error bar against a float32 pipeline and against deliberately wrong oracles, and the host tables the kernels read.

Measured on the test signal (5 280 samples, 34 frames): the float32 NumPy pipeline's live elements use at most 1.5 % of their bar
(the empty rows 40 %: NumPy's float32 log10(1e-10) is one ulp off -10, inside the 4 u |log| of the device function); the
mutations leave it on 56 % (periodic window), 65 % (frames shifted by one sample), 99.8 % (ln for log10) and 9.6 % (reflect that
repeats the edge: the frames that touch the padding) of the live elements; n_frames off by one changes the shape."""

from __future__ import annotations

import numpy as np
import pytest

from tests import audio_ref as R
from tests.conftest import load_golden


@pytest.fixture(scope="module")
def g12():
    return load_golden("g12_whisper_mel.npz")


@pytest.fixture(scope="module")
def whisper_oracle(g12):
    return R.features_oracle(g12["signal"], offset=4.0, scale=0.25)


def test_signal_is_the_recorded_one(g12):
    assert np.array_equal(R.test_signal(5280), g12["signal"]) and np.array_equal(R.test_signal(1600), g12["short"])


def test_filterbank_restatements_equal_the_recorded_one(g12):
    from pygpukit_amd.asr.preprocessing import whisper_mel_filters

    rec = g12["filters"]
    assert rec.shape == (80, 201) and int((rec.sum(axis=1) == 0).sum()) == 4
    assert np.array_equal(whisper_mel_filters(), rec)
    assert np.array_equal(R.whisper_filters(), rec.astype(np.float32))


def test_oracle_reproduces_the_recorded_features(g12):
    """The reference holds its STFT in complex64, so its output is a float32-grade result: it must sit inside the oracle's bar.
    The four empty rows are exactly -10."""
    v, lo, hi = R.features_oracle(g12["signal"])
    assert v.shape == (1, 80, 34)
    assert not R.outside(g12["mel"][None], lo, hi).any()
    assert np.median(np.abs(v[0] - g12["mel"])) < 1e-7
    empty = g12["filters"].sum(axis=1) == 0
    assert (v[0][empty] == -10.0).all() and (g12["mel"][empty] == -10.0).all()
    vn, lon, hin = R.features_oracle(g12["signal"], offset=4.0, scale=0.25)
    assert not R.outside(g12["normalized"][None], lon - 2 ** -22, hin + 2 ** -22).any()       # recorded as float32


def test_oracle_reproduces_the_recorded_padded_run(g12):
    """_preprocess_audio on 1 600 samples: 3001 frames of the zero-padded 30 s; recorded as its first 40 and last 8 frames."""
    x = np.zeros(480000, np.float32)
    x[:1600] = g12["short"]
    fb = g12["filters"].astype(np.float32)
    head, lo, hi = R.features_oracle(x[:40 * 160 + 400], offset=4.0, scale=0.25, fb32=fb)
    assert R.n_frames(480000, 400, 160) == 3001
    slack = 2 ** -22                                                               # the record is float32
    assert not R.outside(g12["first"][None, :, :38], lo[:, :, :38] - slack, hi[:, :, :38] + slack).any()    # frames clear of my cut
    assert (g12["last"] == -1.5).all() and (g12["first"][:, 14:] == -1.5).all()    # silence: log10(1e-10) -> (-10 + 4) / 4


def test_float32_pipeline_stays_inside_the_bar(g12, whisper_oracle):
    v, lo, hi = whisper_oracle
    f32 = R.float32_pipeline(g12["signal"])
    assert not R.outside(f32, lo, hi).any()
    live = v > -1.5
    room = np.maximum(hi - v, v - lo)
    assert (np.abs(f32 - v)[live] / room[live]).max() < 0.05


@pytest.mark.parametrize("mutation, least", [("window_periodic", 0.4), ("shift_one", 0.4), ("ln_for_log10", 0.9), ("reflect_repeats_edge", 0.05),
                                             ("frames_off_by_one", 1.0)])
def test_each_mutation_breaks_the_bar(g12, whisper_oracle, mutation, least):
    v, lo, hi = whisper_oracle
    wrong = R.features_oracle(g12["signal"], offset=4.0, scale=0.25, mutation=mutation)[0]
    out = R.outside(wrong, lo, hi)
    live = v > -1.5
    assert out[live].mean() >= least
    if mutation == "reflect_repeats_edge":                                         # only the frames that touch the padding
        frames = np.flatnonzero(out.any(axis=(0, 1)))
        assert set(frames) <= {0, 1, 32, 33} and {0, 33} <= set(frames)


def test_bar_follows_layout_dtype_and_range(g12):
    x = np.stack([g12["signal"][:1600], 3.0 * g12["signal"][1600:3200]])
    a = R.features_oracle(x, offset=4.0, scale=0.25)
    b = R.features_oracle(x, offset=4.0, scale=0.25, layout="frames_first", dtype="bfloat16")
    assert a[0].shape == (2, 80, 11) and b[0].shape == (2, 11, 80)
    assert np.array_equal(a[0].transpose(0, 2, 1), b[0]) and ((b[2] - b[1]) > (a[2] - a[1]).transpose(0, 2, 1)).all()
    c = R.features_oracle(x, dynamic_range=2.0)
    assert c[0].min() == c[0].max() - 2.0 and R.features_oracle(x)[0].min() == -10.0
    d = R.features_oracle(x, drop_last_frame=True)
    assert d[0].shape == (2, 80, 10) and np.array_equal(d[0], R.features_oracle(x)[0][:, :, :10])


# ------------------------------------------------------------------------------------------------ the tables the kernels read
@pytest.mark.parametrize("n_fft", [16, 18, 400, 512])
def test_host_tables(n_fft):
    from pygpukit_amd.ops.audio import tables as T

    assert np.array_equal(T.window_table("hann", n_fft), R.window("hann", n_fft))
    assert np.array_equal(T.window_table("hann_periodic", n_fft), R.window("hann_periodic", n_fft))
    assert np.array_equal(T.window_table("hann", 400), np.hanning(400).astype(np.float32))
    t = T.dft_table(n_fft)
    n_freq, nbp = n_fft // 2 + 1, T.padded_bins(n_fft)
    assert t.shape == (2, n_fft, nbp) and nbp % 32 == 0 and 0 <= nbp - n_freq < 32 and not t[:, :, n_freq:].any()
    ang = 2 * np.pi * np.arange(n_fft)[:, None] * np.arange(n_freq)[None, :] / n_fft
    assert np.abs(t[0, :, :n_freq] - np.cos(ang)).max() <= 2.0 ** -24 + 1e-12 and np.abs(t[1, :, :n_freq] + np.sin(ang)).max() <= 2.0 ** -24 + 1e-12
    assert (t[0, :, 0] == 1.0).all() and not t[1, :, 0].any() and (t[0, :, n_fft // 2] == np.where(np.arange(n_fft) % 2, -1.0, 1.0)).all()   # integer-reduced angle


def test_htk_filterbank_and_spans():
    from pygpukit_amd.ops.audio import tables as T

    for n_mels, n_fft, sr, f_min, f_max in ((80, 512, 16000, 0.0, -1.0), (5, 16, 16000, 0.0, -1.0), (128, 400, 16000, 0.0, 8000.0), (40, 512, 22050, 50.0, 7000.0)):
        fb = T.mel_filterbank_htk(n_mels, n_fft, sr, f_min, f_max)
        ref = R.htk_filters(n_mels, n_fft, sr, f_min, f_max)
        assert fb.shape == (n_mels, n_fft // 2 + 1) and np.abs(fb.astype(np.float64) - ref).max() <= 2.0 ** -23
        spans = T.filter_spans(fb)
        for row, (lo, hi) in zip(fb, spans):
            nz = np.flatnonzero(row)
            assert (lo, hi) == ((nz[0], nz[-1]) if nz.size else (0, -1))
    from pygpukit_amd.asr.preprocessing import whisper_mel_filters

    assert int((T.filter_spans(whisper_mel_filters())[:, 1] < 0).sum()) == 4


def test_frame_count_and_parameter_checks():
    from pygpukit_amd.ops.audio import tables as T

    assert T.num_frames(480000, 400, 160) == 3001 and T.num_frames(1600, 400, 160) == 11 and T.num_frames(5280, 400, 160) == 34
    assert T.num_frames(150, 400, 160) == 1 and T.num_frames(1600, 400, 160, center=False) == 8 and T.num_frames(1, 16, 16) == 1
    with pytest.raises(ValueError):
        T.num_frames(399, 400, 160, center=False)
    for n_fft, hop in ((401, 160), (14, 4), (4096, 160), (400, 0), (400, 401)):
        with pytest.raises(ValueError):
            T.check_stft_params(n_fft, hop, "t")
    for n_fft, hop in ((400, 160), (16, 16), (2048, 1), (18, 5)):
        T.check_stft_params(n_fft, hop, "t")


@pytest.mark.parametrize("ratio, n_taps", [(3, 32), (2, 22), (6, 64)])
def test_decimator_taps(ratio, n_taps):
    from pygpukit_amd.ops.audio import tables as T

    h = T.decimator_taps(ratio).astype(np.float64)
    assert h.size == n_taps and abs(h.sum() - 1.0) < 1e-6
    assert np.allclose(h[1:], h[1:][::-1], atol=1e-8) and h.argmax() == n_taps // 2          # centred on tap n_taps / 2
    f = np.linspace(0.0, 0.5, 2001)                                                          # cycles per input sample
    H = np.abs(np.exp(-2j * np.pi * f[:, None] * np.arange(n_taps)[None, :]) @ h)
    assert H[f <= 0.2 / ratio].min() > 0.97                                # passband to 0.4 of the output Nyquist rate
    assert H[f >= 0.8 / ratio].max() < 0.02                                # images that would alias below 0.4 of the output rate
    assert T.resampled_length(4801, 48000, 16000) == 1600 and T.resampled_length(441, 44100, 16000) == 160


def test_resample_oracle_lengths_and_tones():
    from pygpukit_amd.ops.audio import tables as T

    x = R.test_signal(1000)
    v, b = R.resample_oracle(x, T.decimator_taps(3), 48000, 16000)
    assert v.size == 333 and b.shape == v.shape and (b > 0).all()
    v, b = R.resample_oracle(x, None, 44100, 16000)
    assert v.size == 1000 * 16000 // 44100 and v[0] == x[0]


def test_plan_and_exports():
    import pygpukit_amd.ops as ops
    from pygpukit_amd.ops import audio

    assert ops.audio is audio and "audio" in ops.__all__ and len(set(ops.__all__)) == len(ops.__all__)
    assert len(set(audio.__all__)) == len(audio.__all__)
    for name in ("AudioBuffer", "from_pcm", "stft", "power_spectrum", "magnitude_spectrum", "create_mel_filterbank", "apply_mel_filterbank",
                 "log_mel", "to_decibels", "mel_spectrogram", "log_mel_spectrogram", "resample", "log_mel_features", "audio_log_mel_plan"):
        assert name in audio.__all__ and hasattr(audio, name), name
    assert audio.audio_log_mel_plan(400, 160) == "lds" and audio.audio_log_mel_plan(512, 160) == "lds"
    assert audio.audio_log_mel_plan(2048, 512) == "global" and audio.audio_log_mel_plan(2048, 512, stage="stft") == "lds"
    with pytest.raises(ValueError):
        audio.audio_log_mel_plan(401, 160)


def test_plan_switch(monkeypatch):
    from pygpukit_amd.ops import audio

    monkeypatch.setenv("PGK_AUDIO_LDS", "0")
    assert audio.audio_log_mel_plan(400, 160) == "global"


def test_preprocessing_constants_and_soundfile_error():
    from pygpukit_amd.asr import preprocessing as P

    assert (P.WHISPER_SAMPLE_RATE, P.WHISPER_N_FFT, P.WHISPER_HOP_LENGTH, P.WHISPER_N_MELS, P.WHISPER_CHUNK_LENGTH, P.WHISPER_N_SAMPLES,
            P.WHISPER_N_FRAMES) == (16000, 400, 160, 80, 30, 480000, 3000)
    try:
        import soundfile  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="soundfile is required"):
            P.preprocess_audio("no_such_file.wav")
