"""float64 oracle of sdpa_mla_prefill (MLA's decompressed form at qk_nope 128 / qk_rope 64 / v 128): per head, plain causal softmax over
[k_nope | kpe], times v.  `rnd` as in mla_ref.op: identity for the exact oracle, rounder(dtype) at P and at the output for the bar's
precondition.  Also the inputs of the GPU tests and the weights of a 4-head layer at these head dims."""

from functools import lru_cache

import numpy as np

from tests import attn_stair_ref as S
from tests import mla_ref as R

NOPE, V = 128, 128
# (S, T, H): the 32-row wave edge, the 128-row query tile edge, the 64-row KV tile edge on both sides, a cached prefix, 1 and 128 heads
SHAPES = [(1, 1, 1), (33, 33, 3), (64, 65, 1), (127, 127, 2), (129, 129, 1), (5, 70, 3), (130, 321, 2), (200, 200, 128)]
LAYER = dict(hidden=128, heads=4, nope=NOPE, v=V)
LAYER_CHUNKS = (70, 3, 1, 1, 1)          # two prompt chunks through forward_prefill, three tokens through forward_fixed_cache


def op(q_nope, q_pe, kv, kpe, scale: float, rnd=R.same) -> np.ndarray:
    """q_nope [S, H, 128], q_pe [S, H, 64], kv [T, H, 256], kpe [T, 64] -> [S, H, 128]; query row i sees keys j <= T - S + i."""
    q_nope, q_pe, kv, kpe = (np.asarray(a, np.float64) for a in (q_nope, q_pe, kv, kpe))
    (s_len, heads, _), t_len = q_nope.shape, kv.shape[0]
    seen = np.arange(t_len)[None, :] <= (t_len - s_len + np.arange(s_len))[:, None]
    out = np.empty((s_len, heads, V))
    for h in range(heads):
        s = np.where(seen, scale * (q_nope[:, h] @ kv[:, h, :NOPE].T + q_pe[:, h] @ kpe.T), -np.inf)
        p = np.exp(s - s.max(axis=1, keepdims=True))
        out[:, h] = rnd(p) @ kv[:, h, NOPE:] / p.sum(axis=1, keepdims=True)
    return rnd(out)


@lru_cache(maxsize=None)
def case(s_len: int, t_len: int, heads: int, dtype: str):
    """(q_nope, q_pe, kv, kpe) of standard-normal values rounded to dtype, read-only: scores have std 1 at R.SCALE."""
    rng = np.random.default_rng(s_len * 100003 + t_len * 1009 + heads + len(dtype))
    shapes = ((s_len, heads, NOPE), (s_len, heads, R.ROPE), (t_len, heads, NOPE + V), (t_len, R.ROPE))
    arrays = tuple(S.round_to(rng.standard_normal(s), dtype).astype(np.float64) for s in shapes)
    for a in arrays:
        a.setflags(write=False)
    return arrays


@lru_cache(maxsize=None)
def exact(s_len: int, t_len: int, heads: int, dtype: str) -> np.ndarray:
    out = op(*case(s_len, t_len, heads, dtype), R.SCALE)
    out.setflags(write=False)
    return out


def make_weights(seed: int, q_lora, dtype: str = "bf16", std: float = 0.05) -> dict:
    """mla_ref.make_weights at LAYER's head dims."""
    rng, (hidden, heads, nope, v) = np.random.default_rng(seed), LAYER.values()
    shapes = dict(kv_a_proj_with_mqa=(R.WIDTH, hidden), kv_b_proj=(heads * (nope + v), R.LATENT), o_proj=(hidden, heads * v))
    shapes.update(dict(q_proj=(heads * (nope + R.ROPE), hidden)) if q_lora is None else
                  dict(q_a_proj=(q_lora, hidden), q_b_proj=(heads * (nope + R.ROPE), q_lora)))
    w = {name: S.round_to(rng.standard_normal(shape) * std, dtype).astype(np.float64) for name, shape in shapes.items()}
    for name, n in (("kv_a_layernorm", R.LATENT),) + ((("q_a_layernorm", q_lora),) if q_lora else ()):
        w[name] = S.round_to(1.0 + 0.1 * rng.standard_normal(n), dtype).astype(np.float64)
    return w
