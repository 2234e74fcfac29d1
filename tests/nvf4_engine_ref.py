"""NumPy side of the engine's NVF4 weights (weight_format "nvf4"): the NK layout the engine streams, restated row by row.

  quantize_nk(W [N, K])     -> data uint8 [N, K/2] (byte j of a row: k = 2j low nibble, 2j+1 high), scale uint8 [N, K/32]
  dequant_nk(data, scale)   -> float32 [N, K] = e2m1(code) * scale value (exact, and exact in bf16)
  transposed_ref(W)         -> the same bytes by way of tests/nvf4_ref.py's reference layout, quantize_nvf4(W.T) transposed

quantize_nk works along the rows directly (its own loop, the block arithmetic of nvf4_ref.scale_byte / code_scaled), so
that comparing it with transposed_ref checks the NK restatement rather than restating the transpose twice."""

from __future__ import annotations

import numpy as np

from oracle import cpu_ref as O
from tests import nvf4_ref as R

F32 = np.float32


def quantize_nk(w: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """W float32 [N, K] (bf16 values), K % 32 == 0 -> (data [N, K/2], scale [N, K/32])."""
    w = np.asarray(w, np.float32)
    N, K = w.shape
    assert K % 32 == 0
    blocks = w.reshape(N, K // 32, 32)
    max_abs = np.fmax.reduce(np.abs(blocks), axis=2, initial=F32(0)).astype(np.float32)   # NaN ignored
    scale = R.scale_byte(max_abs)                                                           # [N, K/32]
    inv = (F32(1) / R.scale_value(scale)).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        codes = R.code_scaled((blocks * inv[:, :, None]).astype(np.float32)).reshape(N, K)
    data = (codes[:, 0::2] | (codes[:, 1::2] << 4)).astype(np.uint8)
    return data, scale


def transposed_ref(w: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    data_kn, scale_kn = R.quantize_nvf4(np.asarray(w, np.float32).T)
    return np.ascontiguousarray(data_kn.T), np.ascontiguousarray(scale_kn.T)


def dequant_nk(data: np.ndarray, scale: np.ndarray) -> np.ndarray:
    data = np.asarray(data, np.uint8)
    N, K = data.shape[0], data.shape[1] * 2
    codes = np.empty((N, K), np.uint8)
    codes[:, 0::2] = data & 15
    codes[:, 1::2] = data >> 4
    return R.E2M1[codes] * np.repeat(R.scale_value(np.asarray(scale, np.uint8).reshape(N, K // 32)), 32, axis=1)


def bf16_round(x: np.ndarray) -> np.ndarray:
    return O.bf16_bits_to_f32(O.f32_to_bf16_bits(np.ascontiguousarray(x, np.float32)))


def layer_shapes(cfg: dict) -> dict[str, tuple[int, int]]:
    H, D, I = cfg["hidden_size"], cfg["head_dim"], cfg["intermediate_size"]
    Hq, Hkv = cfg["num_heads"], cfg["num_kv_heads"]
    return {"w_qkv": ((Hq + 2 * Hkv) * D, H), "w_o": (H, Hq * D), "w_gate_up": (2 * I, H), "w_down": (H, I)}


def random_engine_weights(cfg: dict, seed: int, *, std: float = 0.03, embed_std: float = 0.5) -> dict:
    """Fused engine-layout matrices, N(0, std^2) rounded to bf16 (float32 arrays); norm gammas 1."""
    rng = np.random.default_rng(seed)
    H, D, V = cfg["hidden_size"], cfg["head_dim"], cfg["vocab_size"]
    out = {"embed": bf16_round(rng.standard_normal((V, H), dtype=np.float32) * F32(embed_std)), "layers": []}
    for _ in range(cfg["num_layers"]):
        lw = {n: bf16_round(rng.standard_normal(s, dtype=np.float32) * F32(std)) for n, s in layer_shapes(cfg).items()}
        lw.update(attn_norm=np.ones(H, np.float32), mlp_norm=np.ones(H, np.float32), q_norm=np.ones(D, np.float32),
                  k_norm=np.ones(D, np.float32))
        out["layers"].append(lw)
    out["final_norm"] = np.ones(H, np.float32)
    return out
