"""NumPy restatement of the Llama-4 attention ops and of a tiny Llama-4 text model, written from the formulas:

    l2norm(x)       = x / sqrt(mean(x^2, last axis) + eps)                                   (no gamma)
    t(pos)          = log1p(floor((pos + 1) / floor_scale)) * attn_scale + 1                 (fp32, rounded after every step)
    irope_scale_q   = Q[s, h, :] * t(pos[s])
    sdpa_irope      = softmax(Q K^T * t(pos[i]) / sqrt(D) + mask) V,  mask: kv j visible to row i iff j <= i + causal_offset
    block           = h + o(attn(l2norm(q(n)), l2norm(k(n)), v(n))),  n = rmsnorm(h);  h + down(silu(gate(m)) * up(m)),  m = rmsnorm(h)

Everything but t is evaluated in float64.  tests/golden/g7_llama4.npz holds what the reference's CPU path gives for
the same inputs (tests/golden/gen_llama4_golden.py); tests/test_llama4_cpu.py checks this file against it."""

from __future__ import annotations

import numpy as np

from oracle import cpu_ref as O

TINY_CFG = dict(vocab_size=100, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                num_key_value_heads=2, head_dim=64, rms_norm_eps=1e-5, attn_scale=0.5, floor_scale=4.0, use_qk_norm=True)


def bf16_round(x) -> np.ndarray:
    """float32 values rounded to the nearest bfloat16 (ties to even), as float32."""
    return O.bf16_bits_to_f32(O.f32_to_bf16_bits(np.ascontiguousarray(x, np.float32)))


def bf16_normal(rng, shape, scale: float = 1.0) -> np.ndarray:
    return bf16_round(rng.standard_normal(shape).astype(np.float32) * np.float32(scale))


def l2norm(x, eps: float = 1e-6) -> np.ndarray:
    x = np.asarray(x, np.float64)
    return x / np.sqrt(np.mean(x * x, axis=-1, keepdims=True) + eps)


def irope_temperature(positions, attn_scale: float = 0.1, floor_scale: float = 8192.0) -> np.ndarray:
    """float32, rounded after every step: (float)(pos + 1) / floor_scale, floor, log1p (correctly rounded: evaluated in
    float64, rounded once), * attn_scale, + 1."""
    p1 = (np.asarray(positions).astype(np.int64) + 1).astype(np.float32)
    steps = np.floor(p1 / np.float32(floor_scale)).astype(np.float32)
    lg = np.log1p(steps.astype(np.float64)).astype(np.float32)
    scaled = (lg * np.float32(attn_scale)).astype(np.float32)
    return (scaled + np.float32(1.0)).astype(np.float32)


def irope_scale_q(q, positions, attn_scale: float = 0.1, floor_scale: float = 8192.0) -> np.ndarray:
    """Q [S, H, D] float32 * t: the float32 product, not rounded further."""
    t = irope_temperature(positions, attn_scale, floor_scale)
    return (np.asarray(q, np.float32) * t[:, None, None]).astype(np.float32)


def sdpa_irope(q, k, v, positions, attn_scale: float = 0.1, floor_scale: float = 8192.0, causal_offset: int = 0) -> np.ndarray:
    """Q [Hq, q_len, D], K / V [Hkv, kv_len, D] -> [Hq, q_len, D] float64."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    hq, q_len, d = q.shape
    hkv, kv_len, _ = k.shape
    rep = hq // hkv
    t = irope_temperature(positions, attn_scale, floor_scale).astype(np.float64)
    seen = np.arange(kv_len)[None, :] <= np.arange(q_len)[:, None] + causal_offset
    out = np.empty_like(q)
    for h in range(hq):
        s = (q[h] @ k[h // rep].T) * t[:, None] / np.sqrt(d)
        s = np.where(seen, s, -np.inf)
        p = np.exp(s - s.max(axis=1, keepdims=True))
        out[h] = (p / p.sum(axis=1, keepdims=True)) @ v[h // rep]
    return out


# ---- tiny model ------------------------------------------------------------------------------------------------------

def make_llama4_weights(cfg: dict, seed: int) -> dict:
    """Seeded weights, bf16-representable float32, projections [out, in] (the checkpoint layout)."""
    rng = np.random.default_rng(seed)
    H, I, V = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"]
    nq, nkv = cfg["num_attention_heads"] * cfg["head_dim"], cfg["num_key_value_heads"] * cfg["head_dim"]
    lin = lambda o, i: bf16_normal(rng, (o, i), 1.0 / np.sqrt(i))          # noqa: E731
    gain = lambda n: bf16_round(1.0 + 0.1 * rng.standard_normal(n))          # noqa: E731
    w = {"embed": bf16_normal(rng, (V, H)), "layers": []}
    for _ in range(cfg["num_hidden_layers"]):
        w["layers"].append({"q": lin(nq, H), "k": lin(nkv, H), "v": lin(nkv, H), "o": lin(H, nq), "gate": lin(I, H), "up": lin(I, H),
                            "down": lin(H, I), "input_norm": gain(H), "post_norm": gain(H)})
    w["norm"] = gain(H)
    w["lm_head"] = lin(V, H)
    return w


def checksum(weights) -> float:
    acc, stack = 0.0, [weights]
    while stack:
        w = stack.pop()
        if isinstance(w, dict):
            stack.extend(w[k] for k in sorted(w))
        elif isinstance(w, list):
            stack.extend(w)
        else:
            acc += float(np.sum(np.asarray(w, np.float64)))
    return acc


def hf_tensors(weights: dict) -> dict:
    """{checkpoint tensor name: float32 array} in the Llama-4 naming (language_model.model.*)."""
    t = {"language_model.model.embed_tokens.weight": weights["embed"], "language_model.model.norm.weight": weights["norm"],
         "language_model.lm_head.weight": weights["lm_head"]}
    for i, lw in enumerate(weights["layers"]):
        p = f"language_model.model.layers.{i}"
        for n in "qkvo":
            t[f"{p}.self_attn.{n}_proj.weight"] = lw[n]
        for n in ("gate", "up", "down"):
            t[f"{p}.feed_forward.{n}_proj.weight"] = lw[n]
        t[f"{p}.input_layernorm.weight"] = lw["input_norm"]
        t[f"{p}.post_attention_layernorm.weight"] = lw["post_norm"]
    return t


def _rmsnorm(x, g, eps):
    return x / np.sqrt(np.mean(x * x, axis=-1, keepdims=True) + eps) * g


def forward(cfg: dict, weights: dict, input_ids) -> np.ndarray:
    """logits [S, V] float64."""
    ids = np.asarray(input_ids, np.int64)
    S, Hq, Hkv, D, eps = len(ids), cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["head_dim"], cfg["rms_norm_eps"]
    f = lambda a: np.asarray(a, np.float64)          # noqa: E731
    h = f(weights["embed"])[ids]
    pos = np.arange(S)
    for lw in weights["layers"]:
        n = _rmsnorm(h, f(lw["input_norm"]), eps)
        q, k, v = (n @ f(lw[p]).T for p in "qkv")
        q, k, v = q.reshape(S, Hq, D), k.reshape(S, Hkv, D), v.reshape(S, Hkv, D)
        if cfg["use_qk_norm"]:
            q, k = l2norm(q, eps), l2norm(k, eps)
        a = sdpa_irope(q.transpose(1, 0, 2), k.transpose(1, 0, 2), v.transpose(1, 0, 2), pos, cfg["attn_scale"], cfg["floor_scale"], 0)
        h = h + a.transpose(1, 0, 2).reshape(S, Hq * D) @ f(lw["o"]).T
        m = _rmsnorm(h, f(lw["post_norm"]), eps)
        g = m @ f(lw["gate"]).T
        h = h + (g / (1.0 + np.exp(-g)) * (m @ f(lw["up"]).T)) @ f(lw["down"]).T
    return _rmsnorm(h, f(weights["norm"]), eps) @ f(weights["lm_head"]).T


def generate(cfg: dict, weights: dict, input_ids, max_new_tokens: int):
    """Greedy, re-running forward on the growing sequence: (all token ids, last-row logits of every step)."""
    ids, rows = [int(t) for t in input_ids], []
    for _ in range(max_new_tokens):
        rows.append(forward(cfg, weights, ids)[-1])
        ids.append(int(np.argmax(rows[-1])))
    return np.array(ids, np.int64), np.array(rows)
