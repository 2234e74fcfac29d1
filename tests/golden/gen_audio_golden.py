"""Records tests/golden/g12_whisper_mel.npz from the reference package's own CPU path (its CPU backend: no GPU).

    python tests/golden/gen_audio_golden.py <path to the reference's src directory>

Only this generator imports the reference (`pygpukit`); the tests read the fixture.  Recorded:
  * filters: WhisperModel._create_mel_filterbank(80, 400) [80, 201] float64 (four of its rows are empty);
  * signal, mel: tests/audio_ref.py's test_signal(5280) and WhisperModel._compute_mel_numpy on it, [80, 34] float64 (log10, not
    yet normalised);
  * short, first, last: test_signal(1600) and the first 40 and last 8 frames of WhisperModel._preprocess_audio on it
    ([1, 80, 3001] float32 for the padded 30 s; kept in part so that the file stays small);
  * trimmed_len, padded_tail: asr.preprocessing.pad_or_trim on 1600 samples to 1000 (its length) and to 2000 (its last 400 values);
  * normalized: asr.preprocessing.normalize_mel on mel as float32."""

from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
from tests import audio_ref as R  # noqa: E402


def main() -> None:
    sys.path.insert(0, sys.argv[1])
    from pygpukit.asr.preprocessing import normalize_mel, pad_or_trim
    from pygpukit.asr.whisper.model import WhisperModel

    class Config:
        num_mel_bins = 80

    model = WhisperModel(Config(), None, None)
    signal, short = R.test_signal(5280), R.test_signal(1600)
    mel = model._compute_mel_numpy(signal)
    full = model._preprocess_audio(short).to_numpy()
    assert mel.shape == (80, 34) and full.shape == (1, 80, 3001), (mel.shape, full.shape)
    np.savez_compressed(os.path.join(HERE, "g12_whisper_mel.npz"), filters=model._create_mel_filterbank(80, 400), signal=signal, mel=mel,
                        short=short, first=full[0, :, :40], last=full[0, :, -8:],
                        trimmed_len=np.int64(pad_or_trim(short, 1000).to_numpy().size), padded_tail=pad_or_trim(short, 2000).to_numpy()[-400:],
                        normalized=normalize_mel(mel.astype(np.float32)).to_numpy())


if __name__ == "__main__":
    main()
