"""NumPy restatement of the Llama-4 KV-cache path, built on tests/llama4_ref.py: the same block arithmetic in float64, but
every layer keeps the K (after the L2 norm) and V rows it has seen, and the rows fed now attend over the stored prefix:

    prefill(ids, start_pos)   rows start_pos .. start_pos+S-1 appended, attention = sdpa_irope(q, K[:start_pos+S], V[:start_pos+S],
                              positions start_pos .., causal_offset = start_pos)                  -> logits [S, V]
    step(token, pos)          prefill([token], pos)                                                -> logits [1, V]

Fed the same tokens in any chunking it must reproduce llama4_ref.forward on the whole sequence (tests/test_llama4_cache_cpu.py)."""

from __future__ import annotations

import numpy as np

from tests import llama4_ref as R


class CachedLlama4:
    def __init__(self, cfg: dict, weights: dict):
        self.cfg, self.w = cfg, weights
        hkv, d = cfg["num_key_value_heads"], cfg["head_dim"]
        self.K = [np.zeros((hkv, 0, d)) for _ in weights["layers"]]
        self.V = [np.zeros((hkv, 0, d)) for _ in weights["layers"]]

    def __len__(self) -> int:
        return self.K[0].shape[1]

    def prefill(self, ids, start_pos: int = 0) -> np.ndarray:
        cfg = self.cfg
        ids = np.asarray(ids, np.int64)
        if start_pos != len(self):
            raise ValueError(f"rows must be appended in order: start_pos {start_pos}, cache holds {len(self)}")
        S, Hq, Hkv, D, eps = len(ids), cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["head_dim"], cfg["rms_norm_eps"]
        f = lambda a: np.asarray(a, np.float64)          # noqa: E731
        h = f(self.w["embed"])[ids]
        pos = np.arange(start_pos, start_pos + S)
        for i, lw in enumerate(self.w["layers"]):
            n = R._rmsnorm(h, f(lw["input_norm"]), eps)
            q, k, v = (n @ f(lw[p]).T for p in "qkv")
            q, k, v = q.reshape(S, Hq, D), k.reshape(S, Hkv, D), v.reshape(S, Hkv, D)
            if cfg["use_qk_norm"]:
                q, k = R.l2norm(q, eps), R.l2norm(k, eps)
            self.K[i] = np.concatenate([self.K[i], k.transpose(1, 0, 2)], axis=1)
            self.V[i] = np.concatenate([self.V[i], v.transpose(1, 0, 2)], axis=1)
            a = R.sdpa_irope(q.transpose(1, 0, 2), self.K[i], self.V[i], pos, cfg["attn_scale"], cfg["floor_scale"], start_pos)
            h = h + a.transpose(1, 0, 2).reshape(S, Hq * D) @ f(lw["o"]).T
            m = R._rmsnorm(h, f(lw["post_norm"]), eps)
            g = m @ f(lw["gate"]).T
            h = h + (g / (1.0 + np.exp(-g)) * (m @ f(lw["up"]).T)) @ f(lw["down"]).T
        return R._rmsnorm(h, f(self.w["norm"]), eps) @ f(self.w["lm_head"]).T

    def step(self, token: int, pos: int) -> np.ndarray:
        return self.prefill([int(token)], pos)


def teacher_forced(cfg: dict, weights: dict, ids, prompt_len: int, chunks=None) -> np.ndarray:
    """Logits [len(ids), V]: ids[:prompt_len] prefilled (in `chunks` = row counts summing to prompt_len, default one
    chunk), every later token fed by step() at its position."""
    m = CachedLlama4(cfg, weights)
    rows, at = [], 0
    for n in chunks or [prompt_len]:
        rows.append(m.prefill(ids[at:at + n], at))
        at += n
    assert at == prompt_len
    for p in range(prompt_len, len(ids)):
        rows.append(m.step(ids[p], p))
    return np.concatenate(rows, axis=0)
