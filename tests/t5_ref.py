"""NumPy restatement of T5's relative-position bias, of attention with that bias and of the T5 encoder, in the arithmetic of
`dtype` (float64: the oracle; float32: the yardstick of the float32 bar).  It restates HuggingFace's T5EncoderModel (v1.1: gated
gelu_new FFN, attention scale 1.0) and, with mode="reference", the computation of the reference's T5Encoder CPU path (attention
scale 1/sqrt(d_kv), a ReLU gate, -1e9 on masked keys, 1e-9 added to the softmax denominator).  The fixture
tests/golden/g16_text_encoders.npz (tests/golden/gen_text_encoder_golden.py) holds the outputs of both programs on
make_weights(fixture_config(), seed); tests/test_text_encoders_cpu.py holds this file to it at float64 round-off.

The float32 bar.  A float32 kernel and the float32 restatement below compute the same sums in different orders; each is about as far
from exact arithmetic as the other.  So the bar of a float32 result is the restatement's own distance from the float64 one on the
very inputs of the test, rel_err(ref32, ref64), times 8 for the freedom of summation order (a kernel may add a row's 64..600 terms as
a chain, a tree or lane-strided partial sums; the worst-case bound grows with the chain length, the typical error with its square
root: 8 ~ sqrt(64) covers the gap between this file's pairwise NumPy sums and a chain of a few hundred terms), and never more than
1e-4, the cap tests/test_flux_model_gpu.py applies to float32.  f32_bar() computes it; nothing in it comes from the code under test."""

from __future__ import annotations

import numpy as np

CAP32 = 1e-4
BAR16 = 1e-2


def rel_err(a, b) -> float:
    a = np.asarray(a, np.float64).ravel()
    b = np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def f32_bar(ref32, ref64) -> float:
    return min(CAP32, 8.0 * rel_err(ref32, ref64))


# ---- the bias ----------------------------------------------------------------------------------------------------------

def relpos_bucket(relative_position, bidirectional: bool = True, num_buckets: int = 32, max_distance: int = 128) -> np.ndarray:
    """HF's T5Attention._relative_position_bucket on integers: relative_position = key position - query position."""
    rp = np.asarray(relative_position, np.int64)
    buckets = np.zeros_like(rp)
    if bidirectional:
        num_buckets //= 2
        buckets = buckets + (rp > 0).astype(np.int64) * num_buckets
        rp = np.abs(rp)
    else:
        rp = -np.minimum(rp, 0)
    max_exact = num_buckets // 2
    is_small = rp < max_exact
    safe = np.maximum(rp, 1).astype(np.float32)
    large = max_exact + (np.log(safe / np.float32(max_exact)) / np.float32(np.log(max_distance / max_exact))
                         * np.float32(num_buckets - max_exact)).astype(np.int64)
    large = np.minimum(large, num_buckets - 1)
    return buckets + np.where(is_small, rp, large)


def dense_bias(weight, q_len: int, kv_len: int, bidirectional: bool = True, max_distance: int = 128) -> np.ndarray:
    """weight [num_buckets, H] -> bias [H, q_len, kv_len] = weight[bucket(j - i), h]: what both programs materialise."""
    weight = np.asarray(weight)
    delta = np.arange(kv_len)[None, :] - np.arange(q_len)[:, None]
    return np.transpose(weight[relpos_bucket(delta, bidirectional, weight.shape[0], max_distance)], (2, 0, 1))


def bias_table(weight, bidirectional: bool = True, max_distance: int = 128) -> np.ndarray:
    """weight [num_buckets, H] -> table [H, 2R + 1], R = max_distance: table[h, delta + R] = weight[bucket(delta), h]."""
    weight = np.asarray(weight)
    deltas = np.arange(-max_distance, max_distance + 1)
    return np.ascontiguousarray(weight[relpos_bucket(deltas, bidirectional, weight.shape[0], max_distance)].T)


def expand_table(table, q_len: int, kv_len: int) -> np.ndarray:
    """table [H, 2R + 1] -> [H, q_len, kv_len]: table[h, clamp(j - i, -R, R) + R]."""
    table = np.asarray(table)
    radius = table.shape[1] // 2
    delta = np.arange(kv_len)[None, :] - np.arange(q_len)[:, None]
    return table[:, np.clip(delta, -radius, radius) + radius]


def attention_relbias(q, k, v, table, scale: float = 0.0, dtype=np.float64) -> np.ndarray:
    """q [Hq, q_len, D], k / v [Hkv, kv_len, D], table [Hq, 2R + 1]: softmax(scale q k^T + expand_table) v, no mask."""
    q, k, v, table = (np.asarray(x, dtype) for x in (q, k, v, table))
    hq, q_len, d = q.shape
    hkv, kv_len = k.shape[0], k.shape[1]
    rep = hq // hkv
    sc = dtype(scale if scale > 0 else 1.0 / np.sqrt(d))
    out = np.empty((hq, q_len, d), dtype)
    bias = expand_table(table, q_len, kv_len)
    for h in range(hq):
        s = (q[h] @ k[h // rep].T) * sc + bias[h]
        s = s - s.max(axis=-1, keepdims=True)
        p = np.exp(s)
        out[h] = (p / p.sum(axis=-1, keepdims=True)) @ v[h // rep]
    return out


# ---- the encoder -------------------------------------------------------------------------------------------------------

def fixture_config() -> dict:
    """inner = 3 * 64 = 192 differs from d_model = 128; S = 160 so that |delta| > max_distance occurs; the second element is
    masked to 131 valid tokens (a ragged third KV tile)."""
    return dict(d_model=128, d_kv=64, num_heads=3, d_ff=192, num_layers=2, vocab_size=64, num_buckets=32, max_distance=128,
                batch=2, seq=160, valid=(160, 131), eps=1e-6)


def make_weights(config: dict, seed: int) -> dict:
    """float32 weights under HF's T5EncoderModel names (plus shared.weight), drawn from one generator in a fixed order."""
    rng = np.random.default_rng(seed)
    dm, inner, dff = config["d_model"], config["num_heads"] * config["d_kv"], config["d_ff"]

    def mat(rows, cols, std):
        return (rng.standard_normal((rows, cols)) * std).astype(np.float32)

    w = {"shared.weight": mat(config["vocab_size"], dm, 1.0)}
    w["encoder.embed_tokens.weight"] = w["shared.weight"]
    for i in range(config["num_layers"]):
        p = f"encoder.block.{i}.layer"
        # q / k of this size give scores of a few units at scale 1.0, as trained T5 weights do (its init folds 1/sqrt(d_kv) into q)
        w[f"{p}.0.SelfAttention.q.weight"] = mat(inner, dm, 1.0 / np.sqrt(dm * np.sqrt(config["d_kv"])))
        w[f"{p}.0.SelfAttention.k.weight"] = mat(inner, dm, 1.0 / np.sqrt(dm * np.sqrt(config["d_kv"])))
        w[f"{p}.0.SelfAttention.v.weight"] = mat(inner, dm, 1.0 / np.sqrt(dm))
        w[f"{p}.0.SelfAttention.o.weight"] = mat(dm, inner, 1.0 / np.sqrt(inner))
        if i == 0:
            w[f"{p}.0.SelfAttention.relative_attention_bias.weight"] = mat(config["num_buckets"], config["num_heads"], 1.5)
        w[f"{p}.0.layer_norm.weight"] = (1.0 + 0.1 * rng.standard_normal(dm)).astype(np.float32)
        w[f"{p}.1.DenseReluDense.wi_0.weight"] = mat(dff, dm, 1.0 / np.sqrt(dm))
        w[f"{p}.1.DenseReluDense.wi_1.weight"] = mat(dff, dm, 1.0 / np.sqrt(dm))
        w[f"{p}.1.DenseReluDense.wo.weight"] = mat(dm, dff, 1.0 / np.sqrt(dff))
        w[f"{p}.1.layer_norm.weight"] = (1.0 + 0.1 * rng.standard_normal(dm)).astype(np.float32)
    w["encoder.final_layer_norm.weight"] = (1.0 + 0.1 * rng.standard_normal(dm)).astype(np.float32)
    return w


def make_inputs(config: dict, seed: int):
    """ids [B, S] int64 and the prefix mask [B, S] of config["valid"]."""
    rng = np.random.default_rng(seed + 1000)
    ids = rng.integers(0, config["vocab_size"], (config["batch"], config["seq"])).astype(np.int64)
    mask = (np.arange(config["seq"])[None, :] < np.asarray(config["valid"])[:, None]).astype(np.int64)
    return ids, mask


def _rms(x, g, eps):
    return x / np.sqrt(np.mean(x * x, axis=-1, keepdims=True) + x.dtype.type(eps)) * g


def gelu_new(x):
    return x * x.dtype.type(0.5) * (1 + np.tanh(x.dtype.type(0.7978845608028654) * (x + x.dtype.type(0.044715) * x * x * x)))


def t5_forward(config: dict, weights: dict, ids, mask=None, mode: str = "hf", dtype=np.float64, round_fn=None) -> np.ndarray:
    """[B, S, d_model].  mode "hf": HuggingFace T5 v1.1; "reference": the reference's T5Encoder.  Masked keys are left out of the
    softmax (what finfo.min and -1e9 amount to); every query row, padded ones included, is computed, as both programs do.
    round_fn (optional) rounds the weights and the embedding once, for the 16-bit oracles."""
    rf = round_fn if round_fn is not None else (lambda a: a)
    W = {n: np.asarray(rf(np.asarray(a, np.float32)), dtype) for n, a in weights.items()}
    ids = np.asarray(ids)
    B, S = ids.shape
    H, dk = config["num_heads"], config["d_kv"]
    inner, eps = H * dk, config["eps"]
    scale = 1.0 if mode == "hf" else 1.0 / np.sqrt(dk)
    table = bias_table(W["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"], True, config["max_distance"])
    out = np.empty((B, S, config["d_model"]), dtype)
    for b in range(B):
        n_valid = S if mask is None else int(np.asarray(mask)[b].sum())
        x = W["shared.weight"][ids[b]]
        for i in range(config["num_layers"]):
            p = f"encoder.block.{i}.layer"
            h = _rms(x, W[f"{p}.0.layer_norm.weight"], eps)
            q = (h @ W[f"{p}.0.SelfAttention.q.weight"].T).reshape(S, H, dk).transpose(1, 0, 2)
            k = (h @ W[f"{p}.0.SelfAttention.k.weight"].T).reshape(S, H, dk).transpose(1, 0, 2)
            v = (h @ W[f"{p}.0.SelfAttention.v.weight"].T).reshape(S, H, dk).transpose(1, 0, 2)
            a = attention_relbias(q, k[:, :n_valid], v[:, :n_valid], table, scale, dtype)
            x = x + a.transpose(1, 0, 2).reshape(S, inner) @ W[f"{p}.0.SelfAttention.o.weight"].T
            h = _rms(x, W[f"{p}.1.layer_norm.weight"], eps)
            gate = h @ W[f"{p}.1.DenseReluDense.wi_0.weight"].T
            gate = gelu_new(gate) if mode == "hf" else np.maximum(gate, 0)
            x = x + (gate * (h @ W[f"{p}.1.DenseReluDense.wi_1.weight"].T)) @ W[f"{p}.1.DenseReluDense.wo.weight"].T
        out[b] = _rms(x, W["encoder.final_layer_norm.weight"], eps)
    return out
