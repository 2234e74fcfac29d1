"""pygpukit_amd.ops.audio: sample- and spectrum-domain audio ops for ASR preprocessing (reference: src/pygpukit/ops/audio).

    from pygpukit_amd.ops import audio
    buf = audio.from_pcm(pcm_int16, sample_rate=48000, channels=2).to_mono().resample(16000).normalize()
    mel = audio.log_mel_spectrogram(buf, n_fft=400, hop_length=160, n_mels=80)          # one launch

Here: AudioBuffer / from_pcm, resample, stft, power / magnitude spectrum, mel filterbanks, log_mel, to_decibels, mel_spectrogram,
log_mel_spectrogram and the fused log_mel_features (csrc/ops_audio.hip).  Not here (README): VAD, ring buffer and stream classes,
pre-emphasis and gates, MFCC and delta, iSTFT and Griffin-Lim, pitch, spectral features, CQT and chroma, HPSS, time-stretch and
pitch-shift."""

from pygpukit_amd.ops.audio import tables
from pygpukit_amd.ops.audio.buffer import (AudioBuffer, from_pcm, normalize_peak, normalize_rms, pcm_to_float32, resample,
                                           stereo_to_mono)
from pygpukit_amd.ops.audio.spectral import (MelFilters, apply_mel_filterbank, audio_log_mel_plan, create_mel_filterbank, log_mel,
                                             log_mel_features, log_mel_spectrogram, magnitude_spectrum, mel_spectrogram,
                                             power_spectrum, stft, to_decibels)

__all__ = ["AudioBuffer", "from_pcm", "pcm_to_float32", "stereo_to_mono", "normalize_peak", "normalize_rms", "resample", "stft",
           "power_spectrum", "magnitude_spectrum", "create_mel_filterbank", "apply_mel_filterbank", "log_mel", "to_decibels",
           "mel_spectrogram", "log_mel_spectrogram", "log_mel_features", "audio_log_mel_plan", "MelFilters", "tables"]
