"""float64 oracle of multi-head latent attention (DeepSeek MLA): the op's formula, and the layer in its TEXTBOOK, non-absorbed form
(decompress k_nope = c W_UK^T and v = c W_UV^T per head, concatenate the shared roped key, plain causal softmax attention per head,
o_proj) next to the absorbed form the kernels run.  `rnd` (default: identity) is applied wherever a 16-bit implementation has to
round - the stored result of every op, and P before P.V - so the same code gives the exact oracle and the bar's precondition."""

from __future__ import annotations

import numpy as np

from tests import attn_stair_ref as S

LATENT, ROPE, WIDTH = 512, 64, 576
SCALE = 1.0 / np.sqrt(192.0)         # DeepSeek's 1 / sqrt(qk_nope_head_dim + qk_rope_head_dim) at mscale 1
DECODE_SHAPES = [(1, h, m) for h in (1, 16, 20, 128) for m in (64, 600)]          # (q_len, H, max_seq)
MULTI_SHAPES = [(2, 16, 600), (5, 20, 600), (33, 3, 600)]
LAYER = dict(hidden=128, heads=4, nope=32, v=32)
LAYER_CHUNKS = (12, 3, 1, 1, 1, 1)          # a prompt chunk, a second chunk, four single tokens through the cache
LAYER_SCALE = 1.0 / np.sqrt(32.0 + ROPE)


same = np.asarray         # no rounding: the exact oracle


def rounder(dtype: str):
    return lambda x: S.round_to(x, dtype).astype(np.float64)


def op(q, cache, context_len: int, scale: float, rnd=same) -> np.ndarray:
    """out[i, h] = sum_r softmax_r(scale <q[i, h], cache[r]>) cache[r, :512] over r <= context_len - q_len + i; q [q_len, H, 576]."""
    q, cache = np.asarray(q, np.float64), np.asarray(cache, np.float64)
    out = np.empty(q.shape[:2] + (LATENT,))
    for i in range(q.shape[0]):
        rows = cache[:context_len - q.shape[0] + i + 1]
        s = scale * (q[i] @ rows.T)
        p = np.exp(s - s.max(axis=1, keepdims=True))
        out[i] = rnd(p) @ rows[:, :LATENT] / p.sum(axis=1, keepdims=True)
    return rnd(out)


def case(q_len: int, heads: int, max_seq: int, dtype: str):
    """(q, cache) of standard-normal values rounded to dtype, read-only: scores have std sqrt(576 / 192) = 1.7."""
    rng = np.random.default_rng(q_len * 100003 + heads * 1009 + max_seq + len(dtype))
    q, cache = (S.round_to(rng.standard_normal(s), dtype).astype(np.float64) for s in ((q_len, heads, WIDTH), (max_seq, WIDTH)))
    q.setflags(write=False), cache.setflags(write=False)
    return q, cache


def rope(x, positions, theta: float = 10000.0) -> np.ndarray:
    """Rotate-half RoPE of x [S, ..., 64] at `positions` with the fp32 tables of llm.layers.rope.precompute_freqs_cis."""
    inv = 1.0 / (np.float32(theta) ** (np.arange(0, ROPE, 2, dtype=np.float32) / ROPE))
    ang = np.outer(np.asarray(positions, np.float32), inv)
    shape = (len(positions),) + (1,) * (x.ndim - 2) + (ROPE // 2,)
    c, s = np.cos(ang).astype(np.float64).reshape(shape), np.sin(ang).astype(np.float64).reshape(shape)
    x0, x1 = x[..., :ROPE // 2], x[..., ROPE // 2:]
    return np.concatenate([x0 * c - x1 * s, x1 * c + x0 * s], axis=-1)


def rmsnorm(x, gamma, eps: float) -> np.ndarray:
    return x / np.sqrt((x * x).mean(axis=-1, keepdims=True) + eps) * gamma


def make_weights(seed: int, q_lora: int | None, dtype: str = "bf16", std: float = 0.05) -> dict:
    """The HF-named matrices of a LAYER-sized MLA block, rounded to dtype (float64 values)."""
    rng, (hidden, heads, nope, v) = np.random.default_rng(seed), LAYER.values()
    shapes = dict(kv_a_proj_with_mqa=(WIDTH, hidden), kv_b_proj=(heads * (nope + v), LATENT), o_proj=(hidden, heads * v))
    shapes.update(dict(q_proj=(heads * (nope + ROPE), hidden)) if q_lora is None else
                  dict(q_a_proj=(q_lora, hidden), q_b_proj=(heads * (nope + ROPE), q_lora)))
    w = {name: S.round_to(rng.standard_normal(shape) * std, dtype).astype(np.float64) for name, shape in shapes.items()}
    for name, n in (("kv_a_layernorm", LATENT),) + ((("q_a_layernorm", q_lora),) if q_lora else ()):
        w[name] = S.round_to(1.0 + 0.1 * rng.standard_normal(n), dtype).astype(np.float64)
    return w


def layer_inputs(dtype: str = "bf16") -> list:
    rng = np.random.default_rng(77)
    return [S.round_to(rng.standard_normal((n, LAYER["hidden"])), dtype).astype(np.float64) for n in LAYER_CHUNKS]


class Layer:
    """The layer over a growing cache.  absorbed=False: the textbook form.  absorbed=True: q_abs = q_nope W_UK, `op` over the
    latent rows, o = out W_UV^T - what MLAttention runs, op by op."""

    def __init__(self, w: dict, heads: int, nope: int, v: int, scale: float, eps: float = 1e-6, absorbed: bool = False, rnd=same):
        self.w, self.H, self.nope, self.scale, self.eps, self.absorbed, self.rnd = w, heads, nope, scale, eps, absorbed, rnd
        kvb = w["kv_b_proj"].reshape(heads, nope + v, LATENT)
        self.w_uk, self.w_uv, self.cache = kvb[:, :nope], kvb[:, nope:], np.zeros((0, WIDTH))

    def __call__(self, x) -> np.ndarray:
        w, H, nope, rnd = self.w, self.H, self.nope, self.rnd
        x = np.asarray(x, np.float64)
        n, start = x.shape[0], self.cache.shape[0]
        pos = np.arange(start, start + n)
        xq = x if "q_proj" in w else rnd(rmsnorm(rnd(x @ w["q_a_proj"].T), w["q_a_layernorm"], self.eps))
        q = rnd(xq @ w.get("q_proj", w.get("q_b_proj")).T).reshape(n, H, nope + ROPE)
        q_nope, q_pe = q[..., :nope], rnd(rope(q[..., nope:], pos))
        kv_a = rnd(x @ w["kv_a_proj_with_mqa"].T)         # what mla_cache_write stores: [rmsnorm of the latent | RoPE of the raw shared key]
        rows = rnd(np.concatenate([rmsnorm(kv_a[:, :LATENT], w["kv_a_layernorm"], self.eps), rope(kv_a[:, LATENT:], pos)], axis=1))
        self.cache = np.concatenate([self.cache, rows])
        if self.absorbed:
            q_abs = rnd(np.einsum("shn,hnc->shc", q_nope, self.w_uk))
            out = op(np.concatenate([q_abs, q_pe], axis=-1), self.cache, start + n, self.scale, rnd)
            o = rnd(np.einsum("shc,hvc->shv", out, self.w_uv))
        else:
            c, kpe = self.cache[:, :LATENT], self.cache[:, LATENT:]
            k_nope, val = np.einsum("tc,hnc->thn", c, self.w_uk), np.einsum("tc,hvc->thv", c, self.w_uv)
            s = self.scale * (np.einsum("shn,thn->hst", q_nope, k_nope) + np.einsum("shr,tr->hst", q_pe, kpe))
            s = np.where(np.arange(start + n)[None, None, :] <= pos[None, :, None], s, -np.inf)
            p = np.exp(s - s.max(axis=-1, keepdims=True))
            o = np.einsum("hst,thv->shv", p / p.sum(axis=-1, keepdims=True), val)
        return rnd(o.reshape(n, -1) @ w["o_proj"].T)
