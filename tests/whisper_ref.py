"""NumPy restatement of what conv1d, sdpa_noncausal and the Whisper encoder compute (reference: src/pygpukit/ops/conv.py,
src/pygpukit/asr/whisper/encoder.py; the authority is the reference's own CPU path, recorded in tests/golden/g10_whisper.npz
by gen_whisper_golden.py):

    conv1d     out[b, m, n] = bias[m] + sum_{c, t} w[m, c, t] * x[b, c, n * stride + t - padding]       (direct sum, zero padding)
    attention  softmax(q k^T * scale) v over ALL keys, kv head = q head // (Hq / Hkv)
    encoder    gelu(conv1) -> gelu(conv2, stride 2) -> transpose -> + embed_positions[:seq] -> layers -> layer norm, with
               layer: x += out_proj(attention(q, k, v of layer_norm(x)));  x += fc2(gelu(fc1(layer_norm(x))));  tanh GELU

`dtype` is the type every operand, product and sum is held in: float64 (the oracle) or float32 (the yardstick for what fp32
arithmetic alone costs).  `mutate` plants ONE known error, for the test that shows the bars separate right from wrong."""

from __future__ import annotations

import numpy as np

from tests.attn_stair_ref import from_words, round_to, to_words  # noqa: F401  (re-exported for the GPU tests)

CONV_MUTATIONS = ("drop_tap", "pad_off_by_one", "ignore_stride")
ATTN_MUTATIONS = ("drop_last_key", "extra_padded_key", "causal")

# (B, C_in, C_out, L, K, stride, padding) of tests/test_conv1d_gpu.py with what each reaches; the kernels' tile is 64 output
# channels x 64 positions and the MFMA kernel reduces over chunks of 32 input channels
CONV_CASES = ((1, 16, 32, 64, 3, 1, 1),        # base
              (2, 80, 72, 203, 3, 1, 1),       # ragged C_in, C_out, L; batch offset
              (1, 40, 136, 131, 3, 2, 1),      # stride 2; odd L; C_out over one tile plus a tail
              (1, 8, 8, 9, 1, 1, 0),           # K = 1
              (1, 24, 16, 50, 5, 3, 2),        # K = 5, stride 3, padding 2
              (1, 33, 5, 7, 7, 1, 3),          # C_in odd; window wider than most of the input
              (1, 16, 16, 3, 3, 1, 0),         # L_out = 1
              (1, 100, 70, 300, 3, 2, 1))      # L_out = 150: three position tiles; C_in = 100: four chunks of 32 (13 of 8)

# (Hq, Hkv, q_len, kv_len, D) of tests/test_sdpa_noncausal_gpu.py
ATTN_SHAPES = ((2, 2, 37, 37, 64),             # Whisper fixture shape, one ragged tile
               (4, 2, 130, 200, 128),          # GQA; two query tiles; ragged keys
               (2, 2, 5, 300, 64),             # cross-attention, q_len < kv_len, q_len < 128
               (2, 2, 200, 70, 64),            # q_len > kv_len, which the causal op refuses
               (2, 1, 130, 1000, 64))          # 4 workgroups x 16 KV tiles: KV split + merge kernel


def case_seed(case) -> int:
    return 9000 + sum((i + 1) * 37 * int(v) for i, v in enumerate(case))


def gelu(x):
    """tanh GELU with the reference's constants, in x's dtype."""
    dt = x.dtype.type
    return x * dt(0.5) * (dt(1.0) + np.tanh(dt(0.7978845608) * (x + dt(0.044715) * x * x * x)))


def conv_out_length(L: int, K: int, stride: int, padding: int) -> int:
    return (L + 2 * padding - K) // stride + 1


def conv1d(x, w, b=None, stride=1, padding=0, dtype=np.float64, mutate=None, absolute=False):
    """x [B,C_in,L], w [C_out,C_in,K], b [C_out] or None -> [B,C_out,L_out].  absolute=True returns sum |x w| + |b| instead
    (the scale of the accumulation error bound)."""
    if mutate is not None and mutate not in CONV_MUTATIONS:
        raise ValueError(f"unknown mutation {mutate!r}")
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    if absolute:
        x, w = np.abs(x), np.abs(w)
    B, C_in, L = x.shape
    C_out, _, K = w.shape
    L_out = conv_out_length(L, K, stride, padding)
    assert L_out >= 1
    shift = padding + 1 if mutate == "pad_off_by_one" else padding
    step = 1 if mutate == "ignore_stride" else stride
    xp = np.zeros((B, C_in, L + 2 * padding + K + 1), dtype)                # zeros on both sides, slack for the mutations
    xp[:, :, shift:shift + L] = x
    out = np.zeros((B, C_out, L_out), dtype)
    for t in range(K - 1 if mutate == "drop_tap" else K):
        cols = xp[:, :, t:t + step * (L_out - 1) + 1:step]
        out += np.einsum("mc,bcn->bmn", w[:, :, t], cols)
    if b is not None:
        bb = np.asarray(b, dtype)
        out += (np.abs(bb) if absolute else bb)[None, :, None]
    assert out.dtype == dtype
    return out


def sdpa_noncausal(q, k, v, scale=0.0, dtype=np.float64, mutate=None):
    """q [Hq,q_len,D], k / v [Hkv,kv_len,D] -> [Hq,q_len,D]."""
    if mutate is not None and mutate not in ATTN_MUTATIONS:
        raise ValueError(f"unknown mutation {mutate!r}")
    q, k, v = (np.asarray(a, dtype) for a in (q, k, v))
    hq, q_len, d = q.shape
    rep = hq // k.shape[0]
    k, v = np.repeat(k, rep, axis=0), np.repeat(v, rep, axis=0)
    if mutate == "drop_last_key":
        k, v = k[:, :-1], v[:, :-1]
    if mutate == "extra_padded_key":                      # a zero-filled row of tile padding takes part in the softmax
        k, v = (np.concatenate([a, np.zeros((hq, 1, d), dtype)], axis=1) for a in (k, v))
    s = np.einsum("hqd,hkd->hqk", q, k) * dtype(scale if scale > 0 else 1.0 / np.sqrt(d))
    if mutate == "causal":
        kv_len = k.shape[1]
        s = np.where(np.arange(kv_len)[None, None, :] <= (kv_len - q_len) + np.arange(q_len)[None, :, None], s, -np.inf)
        s[:, np.all(np.isinf(s[0]), axis=1), 0] = 0.0     # q_len > kv_len: a row without keys sees key 0
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    out = np.einsum("hqk,hkd->hqd", p / p.sum(axis=-1, keepdims=True), v)
    assert out.dtype == dtype
    return out


def layernorm(x, gamma, beta, eps=1e-5):
    mu = x.mean(axis=-1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)
    return (x - mu) / np.sqrt(var + x.dtype.type(eps)) * gamma + beta


# ---- encoder -----------------------------------------------------------------------------------------------------------

def make_weights(cfg, seed: int) -> dict:
    """Every encoder tensor under its Hugging Face name, float32, from np.random.default_rng(seed); k_proj has no bias."""
    rng = np.random.default_rng(seed)
    d, f, m = cfg.d_model, cfg.encoder_ffn_dim, cfg.num_mel_bins

    def mat(rows, cols):
        return (rng.standard_normal((rows, cols)) / np.sqrt(cols)).astype(np.float32)

    def vec(n, centre=0.0):
        return (centre + 0.1 * rng.standard_normal(n)).astype(np.float32)

    t = {"model.encoder.conv1.weight": (rng.standard_normal((d, m, 3)) / np.sqrt(3 * m)).astype(np.float32),
         "model.encoder.conv1.bias": vec(d),
         "model.encoder.conv2.weight": (rng.standard_normal((d, d, 3)) / np.sqrt(3 * d)).astype(np.float32),
         "model.encoder.conv2.bias": vec(d),
         "model.encoder.embed_positions.weight": (0.5 * rng.standard_normal((cfg.max_source_positions, d))).astype(np.float32),
         "model.encoder.layer_norm.weight": vec(d, 1.0), "model.encoder.layer_norm.bias": vec(d)}
    for i in range(cfg.encoder_layers):
        p = f"model.encoder.layers.{i}."
        for name in ("q_proj", "k_proj", "v_proj", "out_proj"):
            t[p + f"self_attn.{name}.weight"] = mat(d, d)
            if name != "k_proj":
                t[p + f"self_attn.{name}.bias"] = vec(d)
        t[p + "self_attn_layer_norm.weight"], t[p + "self_attn_layer_norm.bias"] = vec(d, 1.0), vec(d)
        t[p + "fc1.weight"], t[p + "fc1.bias"] = mat(f, d), vec(f)
        t[p + "fc2.weight"], t[p + "fc2.bias"] = mat(d, f), vec(d)
        t[p + "final_layer_norm.weight"], t[p + "final_layer_norm.bias"] = vec(d, 1.0), vec(d)
    return t


def make_mel(cfg, n_frames: int, seed: int, batch: int = 1) -> np.ndarray:
    return np.random.default_rng(seed).standard_normal((batch, cfg.num_mel_bins, n_frames)).astype(np.float32)


def encoder_forward(cfg, tensors: dict, mel, dtype=np.float64, round_dtype: str = "f32"):
    """mel [B, n_mels, n_frames] -> [B, seq, d_model].  round_dtype "bf16" / "f16": weights and mel are first rounded to that
    format (what the device holds); the arithmetic stays in `dtype`."""
    w = {k: np.asarray(round_to(v, round_dtype), dtype) for k, v in tensors.items()}
    x = np.asarray(round_to(mel, round_dtype), dtype)
    e = "model.encoder."
    x = gelu(conv1d(x, w[e + "conv1.weight"], w[e + "conv1.bias"], 1, 1, dtype))
    x = gelu(conv1d(x, w[e + "conv2.weight"], w[e + "conv2.bias"], 2, 1, dtype))
    x = x.transpose(0, 2, 1)
    seq = min(x.shape[1], w[e + "embed_positions.weight"].shape[0])
    x = x[:, :seq] + w[e + "embed_positions.weight"][:seq][None]
    H, d = cfg.encoder_attention_heads, cfg.d_model
    hd = d // H
    zeros = np.zeros(d, dtype)
    for i in range(cfg.encoder_layers):
        p = f"{e}layers.{i}."

        def lin(a, name):
            return a @ w[p + name + ".weight"].T + w.get(p + name + ".bias", zeros if name.endswith("k_proj") else None)

        h = layernorm(x, w[p + "self_attn_layer_norm.weight"], w[p + "self_attn_layer_norm.bias"])
        q, k, v = (lin(h, f"self_attn.{n}_proj").reshape(-1, seq, H, hd).transpose(0, 2, 1, 3) for n in "qkv")
        att = np.stack([sdpa_noncausal(q[b], k[b], v[b], 0.0, dtype) for b in range(x.shape[0])])
        x = x + lin(att.transpose(0, 2, 1, 3).reshape(-1, seq, d), "self_attn.out_proj")
        h = layernorm(x, w[p + "final_layer_norm.weight"], w[p + "final_layer_norm.bias"])
        x = x + lin(gelu(lin(h, "fc1")), "fc2")
    out = layernorm(x, w[e + "layer_norm.weight"], w[e + "layer_norm.bias"])
    assert out.dtype == dtype
    return out


def fixture_config():
    """The configuration tests/golden/g10_whisper.npz was recorded with."""
    from pygpukit_amd.asr.whisper import WhisperConfig

    return WhisperConfig(d_model=128, encoder_layers=2, encoder_attention_heads=2, encoder_ffn_dim=256, num_mel_bins=16,
                         max_source_positions=37)


FIXTURE_SEED, FIXTURE_FRAMES = 1037, 74
# conv cases recorded from the reference's CPU conv1d: (B, C_in, C_out, L, K, stride, padding)
FIXTURE_CONV = ((1, 16, 32, 64, 3, 1, 1), (2, 5, 7, 30, 3, 2, 1), (1, 24, 16, 50, 5, 3, 2), (1, 8, 8, 9, 1, 1, 0), (1, 3, 4, 7, 7, 1, 3))
FIXTURE_ATTN = (3, 5, 11, 16)                  # heads, q_len, kv_len, head_dim of the recorded attention (q_len != kv_len)


def make_conv_case(case, seed=None, bias=True):
    B, C_in, C_out, L, K, _, _ = case
    rng = np.random.default_rng(case_seed(case) if seed is None else seed)
    x = rng.standard_normal((B, C_in, L)).astype(np.float32)
    w = (rng.standard_normal((C_out, C_in, K)) / np.sqrt(C_in * K)).astype(np.float32)
    b = (0.5 * rng.standard_normal(C_out)).astype(np.float32) if bias else None
    return x, w, b


def make_attn_case(shape, seed=None):
    hq, hkv, q_len, kv_len, d = shape
    rng = np.random.default_rng(case_seed(shape) if seed is None else seed)
    return tuple(rng.standard_normal(s).astype(np.float32) for s in ((hq, q_len, d), (hkv, kv_len, d), (hkv, kv_len, d)))
