"""Time Whisper preprocessing of 30 s of audio (480 000 samples -> 3001 frames) three ways, in one process with alternating
windows: per round every variant once, then back through the list (A .. A'), N calls each between device events after a warm-up
of all of them.  Prints medians in us per call, the ratios a / b and a / c, and each variant against itself (A' / A and min..max
of its windows: the margin inside which two numbers are "the same").  80 and 128 mels, float32 and bfloat16 out.

  (a) asr.preprocessing.preprocess_audio on samples already on the device: the fused log-mel kernel, one launch
  (b) the composition of this project's unfused ops: stft, power_spectrum, apply_mel_filterbank (float32 matmul_nt), clamp + log10
      as to_decibels / 10, the affine through the elementwise ops, transpose, cast - the same window and filterbank
  (c) the reference's way: the features in NumPy on the host (vectorised, not its Python loop over 3001 frames, which takes
      seconds) plus the upload; timed with the host clock, includes the device -> host copy of the padded samples as the
      reference does
  (d) WhisperModel.transcribe on a synthetic 2-layer model (d_model 384, 12 generated tokens), with preprocessing's share
(a) is first checked against (b) and (c) (largest absolute difference of the normalised log-mel).
usage: audio_bench.py [--rounds N]"""
import ctypes as C, os, statistics, sys, time, numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from pygpukit_amd import _hip, ops
from pygpukit_amd.asr import preprocessing as P
from pygpukit_amd.asr.whisper import WhisperConfig, WhisperModel, WhisperWeights, create_decoder, create_encoder
from pygpukit_amd.core import GPUArray, bfloat16, float32, from_numpy
from pygpukit_amd.ops import audio

N = P.WHISPER_N_SAMPLES


def host(a):
    h = a.to_numpy()
    return (h.astype(np.uint32) << 16).view(np.float32) if h.dtype == np.uint16 else h.astype(np.float32)


def window_us(run, e0, e1, n, wall=False):
    if wall:
        _hip.call("pgk_device_sync"); t = time.perf_counter()
        for _ in range(n): run()
        _hip.call("pgk_device_sync"); return (time.perf_counter() - t) * 1e6 / n
    _hip.call("pgk_event_record", e0, None)
    for _ in range(n): run()
    _hip.call("pgk_event_record", e1, None); _hip.call("pgk_event_sync", e1)
    ms = C.c_float(); _hip.call("pgk_event_elapsed_ms", e0, e1, C.byref(ms))
    return ms.value * 1000 / n


def race(variants, e0, e1, rounds):
    """variants: [(name, run, calls per window, host clock?)] -> {name: (median us, A'/A, min, max)}"""
    for _, run, _, _ in variants:
        for _ in range(3): run()
    _hip.call("pgk_device_sync")
    first, second = {v[0]: [] for v in variants}, {v[0]: [] for v in variants}
    for _ in range(rounds):
        for name, run, n, wall in variants: first[name].append(window_us(run, e0, e1, n, wall))
        for name, run, n, wall in reversed(variants): second[name].append(window_us(run, e0, e1, n, wall))
    med = statistics.median
    return {v[0]: (med(first[v[0]] + second[v[0]]), med(second[v[0]]) / med(first[v[0]]), min(first[v[0]] + second[v[0]]),
                   max(first[v[0]] + second[v[0]])) for v in variants}


def show(title, res):
    print(title, flush=True)
    for name, (m, self_ratio, lo, hi) in res.items():
        print(f"    {name:<34} {m:10.1f} us   (against itself A'/A {self_ratio:6.4f}, windows {lo:.1f} .. {hi:.1f} us)", flush=True)


def unfused(x, fb_dev, n_mels, dtype, four, quarter):
    """The same features on the unfused ops.  stft applies the periodic window, so (a) is run with it too in the comparison."""
    mel = audio.apply_mel_filterbank(audio.power_spectrum(audio.stft(x, n_fft=400, hop_length=160)), fb_dev)       # [3001, n_mels]
    db = audio.to_decibels(ops.clamp(mel, 1e-10, 3.0e38), eps=0.0)                                                  # 10 log10(max(m, eps))
    out = ops.transpose(ops.mul(ops.add(ops.mul(db, four[1]), four[0]), quarter))                                   # (x / 10 + 4) / 4
    return out if dtype is float32 else out.astype(dtype)


def numpy_features(x_dev, window, fb):
    x = x_dev.to_numpy()
    pad = np.pad(x, 200, mode="reflect")
    frames = np.lib.stride_tricks.sliding_window_view(pad, 400)[::160] * window
    power = np.abs(np.fft.rfft(frames, axis=1)) ** 2
    mel = np.log10(np.clip(fb @ power.T, 1e-10, None))
    return from_numpy(((mel + 4.0) / 4.0).astype(np.float32)[None])


def features(e0, e1, rounds):
    x = from_numpy((0.1 * np.random.default_rng(0).standard_normal(N)).astype(np.float32))
    for n_mels in (80, 128):
        fb = P.whisper_mel_filters(n_mels)
        fb_dev = from_numpy(fb.astype(np.float32))
        shape = (3001, n_mels)
        four = (from_numpy(np.full(shape, 4.0, np.float32)), from_numpy(np.full(shape, 0.1, np.float32)))
        quarter = from_numpy(np.full(shape, 0.25, np.float32))
        win64 = np.hanning(400)
        a_periodic = host(P.preprocess_audio(x, n_mels=n_mels, window="hann_periodic"))
        print(f"{n_mels} mels: fused vs unfused ops (periodic window) max |diff| {np.abs(a_periodic - host(unfused(x, fb_dev, n_mels, float32, four, quarter))).max():.2e}; "
              f"fused vs host NumPy {np.abs(host(P.preprocess_audio(x, n_mels=n_mels)) - host(numpy_features(x, win64, fb))[0]).max():.2e}", flush=True)
        for dtype in (float32, bfloat16):
            res = race([("(a) preprocess_audio, fused", lambda: P.preprocess_audio(x, n_mels=n_mels, dtype=dtype), 50, False),
                        ("(b) unfused ops", lambda: unfused(x, fb_dev, n_mels, dtype, four, quarter), 20, False),
                        ("(c) host NumPy + upload", lambda: numpy_features(x, win64, fb), 2, True)], e0, e1, rounds)
            show(f"30 s, {n_mels} mels, {dtype.name} out, us per call:", res)
            a, b, c = (res[k][0] for k in res)
            print(f"    a / b {a / b:.4f}   a / c {a / c:.5f}", flush=True)


def transcribe(e0, e1, rounds):
    d, ffn, vocab = 384, 1536, 51865
    cfg = WhisperConfig(d_model=d, encoder_layers=2, decoder_layers=2, encoder_attention_heads=6, decoder_attention_heads=6,
                        encoder_ffn_dim=ffn, decoder_ffn_dim=ffn, vocab_size=vocab, num_mel_bins=80, max_source_positions=1500,
                        max_target_positions=448, eos_token_id=vocab - 1, decoder_start_token_id=vocab - 2)
    rng = np.random.default_rng(1)
    mat = lambda r, c: rng.standard_normal((r, c), dtype=np.float32) / np.float32(np.sqrt(c))
    vec = lambda n, m=0.0: (m + 0.1 * rng.standard_normal(n)).astype(np.float32)

    def layer(kinds):
        w = {}
        for a in kinds:
            for p in ("q", "k", "v", "out"):
                w[f"{a}_{p}_weight"], w[f"{a}_{p}_bias"] = mat(d, d), (None if p == "k" else vec(d))
            w[f"{a}_layer_norm_weight"], w[f"{a}_layer_norm_bias"] = vec(d, 1.0), vec(d)
        w.update(fc1_weight=mat(ffn, d), fc1_bias=vec(ffn), fc2_weight=mat(d, ffn), fc2_bias=vec(d), final_layer_norm_weight=vec(d, 1.0),
                 final_layer_norm_bias=vec(d))
        return w

    w = WhisperWeights(cfg)
    w.encoder_conv1_weight, w.encoder_conv1_bias = 0.05 * rng.standard_normal((d, 80, 3), dtype=np.float32), vec(d)
    w.encoder_conv2_weight, w.encoder_conv2_bias = 0.03 * rng.standard_normal((d, d, 3), dtype=np.float32), vec(d)
    w.encoder_embed_positions = 0.1 * rng.standard_normal((1500, d), dtype=np.float32)
    w.encoder_layer_norm_weight, w.encoder_layer_norm_bias = vec(d, 1.0), vec(d)
    w.encoder_layers = [layer(("self_attn",)) for _ in range(2)]
    w.decoder_embed_tokens, w.decoder_embed_positions = rng.standard_normal((vocab, d), dtype=np.float32), rng.standard_normal((448, d), dtype=np.float32)
    w.decoder_layer_norm_weight, w.decoder_layer_norm_bias, w.proj_out_weight = vec(d, 1.0), vec(d), mat(vocab, d)
    w.decoder_layers = [layer(("self_attn", "cross_attn")) for _ in range(2)]
    model = WhisperModel(cfg, create_encoder(cfg, w, bfloat16), create_decoder(cfg, w, bfloat16))
    x = (0.1 * rng.standard_normal(N)).astype(np.float32)
    xd = from_numpy(x)
    tokens = model.transcribe(xd, max_length=12).segments[0].tokens
    res = race([("(d) transcribe, samples on device", lambda: model.transcribe(xd, max_length=12), 3, True),
                ("    preprocessing alone (bf16)", lambda: model._preprocess_audio(xd), 50, False),
                ("    transcribe from host samples", lambda: model.transcribe(x, max_length=12), 3, True)], e0, e1, rounds)
    show(f"transcribe, 2 + 2 layers, d_model {d}, bf16, {len(tokens)} tokens, us per call (host clock for transcribe):", res)
    t, p = res["(d) transcribe, samples on device"][0], res["    preprocessing alone (bf16)"][0]
    print(f"    preprocessing's share of transcribe: {100 * p / t:.2f} %", flush=True)


def main():
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 7
    e0, e1 = C.c_void_p(), C.c_void_p()
    _hip.call("pgk_event_create", C.byref(e0)); _hip.call("pgk_event_create", C.byref(e1))
    print(f"fused kernel plan at 400 / 160: samples from {audio.audio_log_mel_plan(400, 160)}", flush=True)
    features(e0, e1, rounds)
    transcribe(e0, e1, rounds)


if __name__ == "__main__":
    main()
