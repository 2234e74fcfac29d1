"""WhisperModel without a device: preprocessing, encoder and decoder are stubs, so what is checked is the model's own logic - the
chunk arithmetic of transcribe_streaming, the segment fields, the token fallback string, the tokenizer wrapper and the exports."""

from __future__ import annotations

import json

import numpy as np
import pytest

from pygpukit_amd.asr.whisper.model import TranscriptionResult, TranscriptionSegment, WhisperModel, WhisperTokenizer


class _Encoder:
    dtype = "float32"

    def __call__(self, mel):
        return ("encoded", mel)


class _Decoder:
    def __init__(self):
        self.calls = []

    def generate(self, encoder_output, max_length=448, temperature=1.0, top_k=None):
        self.calls.append(dict(n=encoder_output[1], max_length=max_length, temperature=temperature, top_k=top_k))
        return [201, len(self.calls), encoder_output[1] % 200]


def _model(monkeypatch, tokenizer=None):
    model = WhisperModel(config=None, encoder=_Encoder(), decoder=_Decoder(), tokenizer=tokenizer)
    monkeypatch.setattr(model, "_preprocess_audio", lambda samples: len(samples))          # the "mel" is the chunk's length
    return model


def test_transcribe_returns_one_segment_spanning_the_input(monkeypatch):
    model = _model(monkeypatch)
    res = model.transcribe(np.zeros(24000, np.float32), language="ja", max_length=30)
    assert isinstance(res, TranscriptionResult) and res.language == "ja" and len(res.segments) == 1
    seg = res.segments[0]
    assert isinstance(seg, TranscriptionSegment) and (seg.start, seg.end) == (0.0, 1.5) and seg.tokens == [201, 1, 24000 % 200]
    assert res.text == seg.text == "<tokens: [201, 1, 0]>"                                 # no tokenizer: the reference's fallback
    assert model.decoder.calls == [dict(n=24000, max_length=30, temperature=0.0, top_k=None)]
    model.transcribe(np.zeros(16000, np.float32), temperature=0.7)
    assert model.decoder.calls[1] == dict(n=16000, max_length=448, temperature=0.7, top_k=50)


@pytest.mark.parametrize("seconds, chunk, overlap, want", [
    (70.0, 30, 0.0, [(0.0, 30.0), (30.0, 60.0), (60.0, 70.0)]),                            # a short last chunk
    (60.0, 30, 0.0, [(0.0, 30.0), (30.0, 60.0)]),                                          # no empty chunk at the end
    (70.0, 30, 5.0, [(0.0, 30.0), (25.0, 55.0), (50.0, 70.0)]),                            # chunks start chunk - overlap apart
    (2.5, 1.0, 0.25, [(0.0, 1.0), (0.75, 1.75), (1.5, 2.5), (2.25, 2.5)]),
    (10.0, 30, 0.0, [(0.0, 10.0)]),
])
def test_streaming_chunk_starts_and_ends(monkeypatch, seconds, chunk, overlap, want):
    model = _model(monkeypatch)
    segs = list(model.transcribe_streaming(np.zeros(int(seconds * 16000), np.float32), chunk_length=chunk, overlap=overlap, max_length=12))
    assert [(s.start, s.end) for s in segs] == want
    assert [c["n"] for c in model.decoder.calls] == [int(round((e - s) * 16000)) for s, e in want]
    assert all(c["max_length"] == 12 and c["top_k"] is None for c in model.decoder.calls)
    assert [s.tokens[1] for s in segs] == list(range(1, len(want) + 1)) and all(s.text == f"<tokens: {s.tokens}>" for s in segs)


def test_streaming_rejects_an_overlap_that_never_advances(monkeypatch):
    with pytest.raises(ValueError):
        list(_model(monkeypatch).transcribe_streaming(np.zeros(16000, np.float32), chunk_length=1.0, overlap=1.0))


def test_tokenizer_round_trip_and_fallback(tmp_path, monkeypatch):
    missing = WhisperTokenizer(str(tmp_path))                                              # no tokenizer.json there
    assert not missing.available
    with pytest.raises(RuntimeError, match="Tokenizer not available"):
        missing.decode([1, 2])
    assert _model(monkeypatch, tokenizer=missing).transcribe(np.zeros(1600, np.float32)).text.startswith("<tokens: [201, 1,")
    pytest.importorskip("tokenizers")
    vocab = {"[UNK]": 0, "<|startoftranscript|>": 1, "hello": 2, "world": 3, "again": 4}
    spec = {"version": "1.0", "truncation": None, "padding": None,
            "added_tokens": [{"id": 1, "content": "<|startoftranscript|>", "single_word": False, "lstrip": False, "rstrip": False,
                              "normalized": False, "special": True}],
            "normalizer": None, "pre_tokenizer": {"type": "Whitespace"}, "post_processor": None, "decoder": None,
            "model": {"type": "WordLevel", "vocab": vocab, "unk_token": "[UNK]"}}
    (tmp_path / "tokenizer.json").write_text(json.dumps(spec))
    tok = WhisperTokenizer(str(tmp_path))
    assert tok.available and tok.encode("hello world again") == [2, 3, 4]
    assert tok.decode([1, 2, 3]) == "hello world" and "startoftranscript" in tok.decode([1, 2], skip_special_tokens=False)

    class _Fixed(_Decoder):
        def generate(self, *a, **k):
            return [1, 2, 3, 4]

    model = _model(monkeypatch, tokenizer=tok)
    model.decoder = _Fixed()
    assert model.transcribe(np.zeros(1600, np.float32)).text == "hello world again"


def test_from_pretrained_points_at_from_tensors():
    with pytest.raises(NotImplementedError, match="WhisperWeights.from_tensors"):
        WhisperModel.from_pretrained("openai/whisper-tiny")


def test_exports():
    import pygpukit_amd.asr as asr
    from pygpukit_amd.asr import preprocessing, whisper

    for name in ("WhisperModel", "WhisperTokenizer", "TranscriptionResult", "TranscriptionSegment"):
        assert getattr(whisper, name) is getattr(asr, name) and name in whisper.__all__ and name in asr.__all__
    for name in ("preprocess_audio", "preprocess_audio_batch", "pad_or_trim", "normalize_mel", "WHISPER_SAMPLE_RATE", "WHISPER_N_FFT",
                 "WHISPER_HOP_LENGTH", "WHISPER_N_MELS", "WHISPER_CHUNK_LENGTH", "WHISPER_N_SAMPLES", "WHISPER_N_FRAMES"):
        assert getattr(asr, name) is getattr(preprocessing, name) and name in asr.__all__ and name in preprocessing.__all__
    assert len(set(asr.__all__)) == len(asr.__all__) and len(set(whisper.__all__)) == len(whisper.__all__)
