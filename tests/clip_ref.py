"""NumPy restatement of HuggingFace's CLIPTextModel (pre-LN blocks, biased projections, causal attention, quick_gelu or gelu MLP,
final LayerNorm, pooled output at the first EOS) in the arithmetic of `dtype`.  tests/golden/g16_text_encoders.npz holds
transformers' float64 outputs on make_weights(fixture_config(), seed); tests/test_text_encoders_cpu.py holds this file to them."""

from __future__ import annotations

import numpy as np

PREFIX = "text_model."


def fixture_config() -> dict:
    """Two heads of 64; row 0 has its EOS early (position 9, padding after it), row 1 has it last (position 76)."""
    return dict(hidden_size=128, num_heads=2, num_layers=2, intermediate_size=256, vocab_size=96, max_positions=77, hidden_act="quick_gelu",
                eos_token_id=95, bos_token_id=94, pad_token_id=0, batch=2, seq=77, eos_at=(9, 76), eps=1e-5)


def make_weights(config: dict, seed: int) -> dict:
    """float32 weights under the checkpoint names (with the text_model. prefix), drawn from one generator in a fixed order."""
    rng = np.random.default_rng(seed)
    d, dff = config["hidden_size"], config["intermediate_size"]

    def mat(rows, cols, std):
        return (rng.standard_normal((rows, cols)) * std).astype(np.float32)

    def vec(n, mean, std):
        return (mean + std * rng.standard_normal(n)).astype(np.float32)

    w = {PREFIX + "embeddings.token_embedding.weight": mat(config["vocab_size"], d, 1.0),
         PREFIX + "embeddings.position_embedding.weight": mat(config["max_positions"], d, 0.5)}
    for i in range(config["num_layers"]):
        p = f"{PREFIX}encoder.layers.{i}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            w[f"{p}self_attn.{n}.weight"] = mat(d, d, (2.0 if n in ("q_proj", "k_proj") else 1.0) / np.sqrt(d))
            w[f"{p}self_attn.{n}.bias"] = vec(d, 0.0, 0.1)
        w[p + "layer_norm1.weight"], w[p + "layer_norm1.bias"] = vec(d, 1.0, 0.1), vec(d, 0.0, 0.1)
        w[p + "mlp.fc1.weight"], w[p + "mlp.fc1.bias"] = mat(dff, d, 1.0 / np.sqrt(d)), vec(dff, 0.0, 0.1)
        w[p + "mlp.fc2.weight"], w[p + "mlp.fc2.bias"] = mat(d, dff, 1.0 / np.sqrt(dff)), vec(d, 0.0, 0.1)
        w[p + "layer_norm2.weight"], w[p + "layer_norm2.bias"] = vec(d, 1.0, 0.1), vec(d, 0.0, 0.1)
    w[PREFIX + "final_layer_norm.weight"], w[PREFIX + "final_layer_norm.bias"] = vec(d, 1.0, 0.1), vec(d, 0.0, 0.1)
    return w


def make_inputs(config: dict, seed: int):
    """ids [B, S]: BOS, tokens below BOS, EOS at config["eos_at"], pad after it; and the matching prefix mask."""
    rng = np.random.default_rng(seed + 1000)
    B, S = config["batch"], config["seq"]
    ids = np.full((B, S), config["pad_token_id"], np.int64)
    mask = np.zeros((B, S), np.int64)
    for b, e in enumerate(config["eos_at"]):
        ids[b, 0] = config["bos_token_id"]
        ids[b, 1:e] = rng.integers(1, config["bos_token_id"], e - 1)
        ids[b, e] = config["eos_token_id"]
        mask[b, :e + 1] = 1
    return ids, mask


def pooled_position(ids_row, eos_token_id: int) -> int:
    """HF's rule: argmax of the ids when eos_token_id == 2 (old configs, where the EOS is the largest id), else the first EOS."""
    ids_row = np.asarray(ids_row)
    if eos_token_id == 2:
        return int(np.argmax(ids_row))
    return int(np.argmax(ids_row == eos_token_id))


def _ln(x, g, b, eps):
    mu = x.mean(axis=-1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)
    return (x - mu) / np.sqrt(var + x.dtype.type(eps)) * g + b


def _act(x, name):
    if name == "quick_gelu":
        return x / (1 + np.exp(-x.dtype.type(1.702) * x))
    if name == "gelu":      # erf form
        from math import erf
        return x * x.dtype.type(0.5) * (1 + np.vectorize(erf)(x / np.sqrt(2.0)).astype(x.dtype))
    raise ValueError(name)


def clip_forward(config: dict, weights: dict, ids, dtype=np.float64, round_fn=None):
    """-> (last_hidden_state [B, S, hidden], pooled [B, hidden])."""
    rf = round_fn if round_fn is not None else (lambda a: a)
    W = {n: np.asarray(rf(np.asarray(a, np.float32)), dtype) for n, a in weights.items()}
    ids = np.asarray(ids)
    B, S = ids.shape
    d, H = config["hidden_size"], config["num_heads"]
    hd, eps = d // H, config["eps"]
    causal = np.triu(np.ones((S, S), bool), 1)
    hidden = np.empty((B, S, d), dtype)
    pooled = np.empty((B, d), dtype)
    for b in range(B):
        x = W[PREFIX + "embeddings.token_embedding.weight"][ids[b]] + W[PREFIX + "embeddings.position_embedding.weight"][:S]
        for i in range(config["num_layers"]):
            p = f"{PREFIX}encoder.layers.{i}."
            h = _ln(x, W[p + "layer_norm1.weight"], W[p + "layer_norm1.bias"], eps)
            q, k, v = ((h @ W[f"{p}self_attn.{n}.weight"].T + W[f"{p}self_attn.{n}.bias"]).reshape(S, H, hd).transpose(1, 0, 2)
                       for n in ("q_proj", "k_proj", "v_proj"))
            s = q @ k.transpose(0, 2, 1) * dtype(1.0 / np.sqrt(hd))
            s = np.where(causal[None], -np.inf, s)
            s = s - s.max(axis=-1, keepdims=True)
            pr = np.exp(s)
            a = (pr / pr.sum(axis=-1, keepdims=True)) @ v
            x = x + a.transpose(1, 0, 2).reshape(S, d) @ W[p + "self_attn.out_proj.weight"].T + W[p + "self_attn.out_proj.bias"]
            h = _ln(x, W[p + "layer_norm2.weight"], W[p + "layer_norm2.bias"], eps)
            h = _act(h @ W[p + "mlp.fc1.weight"].T + W[p + "mlp.fc1.bias"], config["hidden_act"])
            x = x + h @ W[p + "mlp.fc2.weight"].T + W[p + "mlp.fc2.bias"]
        hidden[b] = _ln(x, W[PREFIX + "final_layer_norm.weight"], W[PREFIX + "final_layer_norm.bias"], eps)
        pooled[b] = hidden[b, pooled_position(ids[b], config["eos_token_id"])]
    return hidden, pooled
