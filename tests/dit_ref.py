"""NumPy statement of the diffusion-transformer ops and of the PixArt forward (pygpukit_amd.diffusion), the oracle of the DiT
tests.  Every function takes the arithmetic dtype (`np.float64` for the truth, `np.float32` for the float32 yardstick) and, where
the device holds 16-bit data, `round_dtype` ("bf16" / "f16") rounds exactly those inputs first.  Nothing here imports the code
under test, the reference package or oracle/.

The forward follows the reference's models/dit/*.py step by step, quirks included: the model's sinusoidal embedding is [sin | cos]
with divisor half_dim - 1, the 2-D position table flattens its grid column-major while patches are row-major, LayerNorm eps is
1e-6, SiLU precedes adaln_single.linear, cross-attention is neither modulated nor gated, the final layer's shift is table[0] +
t_emb and its scale table[1].  One deliberate difference: the softmax denominator carries no `+ 1e-9` (the reference's adds one;
with the row maximum subtracted the sum is >= 1, so the relative change is <= 1e-9, two orders below the float32 yardstick)."""

from __future__ import annotations

import dataclasses
import math

import numpy as np

F32 = np.float32


# ---- number formats -------------------------------------------------------------------------------------------------------------
def _bf16_bits(x) -> np.ndarray:
    u = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)        # round to nearest even (finite inputs)


def round_to(x, dtype: str) -> np.ndarray:
    """Values -> the nearest value of "f32" / "f16" / "bf16" (ties to even), as float32."""
    x = np.ascontiguousarray(x, F32)
    if dtype == "f32":
        return x
    if dtype == "f16":
        return x.astype(np.float16).astype(F32)
    assert dtype == "bf16", dtype
    return (_bf16_bits(x).astype(np.uint32) << 16).view(F32)


def to_words(x, dtype: str) -> np.ndarray:
    """What the device holds: uint16 words for bf16, float16 for f16, the float32 array for f32."""
    x = np.ascontiguousarray(x, F32)
    if dtype == "f32":
        return x
    return _bf16_bits(x) if dtype == "bf16" else x.astype(np.float16)


def from_words(w, dtype: str) -> np.ndarray:
    if dtype == "bf16":
        return (np.ascontiguousarray(w).view(np.uint16).astype(np.uint32) << 16).view(F32)
    return np.asarray(w).astype(F32)


ULP = {"f32": 2.0 ** -23, "f16": 2.0 ** -10, "bf16": 2.0 ** -7}      # one unit in the last place, relative to |value|


# ---- the row ops ----------------------------------------------------------------------------------------------------------------
def layer_norm(x, eps=1e-6):
    """(x - mean) / sqrt(var + eps) over the last axis: population variance, no gamma / beta."""
    dt = x.dtype.type
    mean = x.mean(axis=-1, keepdims=True)
    d = x - mean
    var = (d * d).mean(axis=-1, keepdims=True)
    return d / np.sqrt(var + dt(eps))


def mod_vector(table, vec, batch: int, features: int, default: float, dtype=np.float64):
    """table [D] + vec [B, D] (or [D], shared), either absent -> [B, 1, D]; `default` when both are."""
    if table is None and vec is None:
        return np.full((batch, 1, features), default, dtype)
    out = np.zeros((batch, features), dtype)
    if table is not None:
        out = out + np.asarray(table, dtype).reshape(1, features)
    if vec is not None:
        out = out + np.asarray(vec, dtype).reshape(-1, features)
    return out[:, None, :]


def fused(x, residual=None, gate=None, scale=None, shift=None, eps=1e-6, norm=True, dtype=np.float64):
    """The fused form: s = residual + gate * x (or x); y = (norm ? LN(s) : s) * (1 + scale) + shift.  gate / scale / shift are
    (table, vec) pairs or None.  Returns (s, y) unrounded."""
    x = np.asarray(x, dtype)
    B, _, D = x.shape
    s = x
    if residual is not None:
        s = np.asarray(residual, dtype) + mod_vector(*(gate or (None, None)), B, D, 1.0, dtype) * x
    n = layer_norm(s, eps) if norm else s
    y = n * (1 + mod_vector(*(scale or (None, None)), B, D, 0.0, dtype)) + mod_vector(*(shift or (None, None)), B, D, 0.0, dtype)
    return s, y


def adaln(x, scale, shift, eps=1e-5, dtype=np.float64):
    """The reference's diffusion/ops adaln: (1 + scale) * LN(x) + shift, vectors [B, D]."""
    return fused(x, None, None, (None, scale), (None, shift), eps, True, dtype)[1]


def adaln_zero(x, scale, shift, gate, residual, eps=1e-5, dtype=np.float64):
    """The reference's adaln_zero: residual + gate * ((1 + scale) * LN(x) + shift)."""
    x = np.asarray(x, dtype)
    B, _, D = x.shape
    return np.asarray(residual, dtype) + mod_vector(None, gate, B, D, 1.0, dtype) * adaln(x, scale, shift, eps, dtype)


def attention(q, k, v, scale=0.0, dtype=np.float64):
    """softmax(q k^T * scale) v on [..., N, D]; scale <= 0 -> 1 / sqrt(D)."""
    q, k, v = (np.asarray(a, dtype) for a in (q, k, v))
    if scale <= 0:
        scale = 1.0 / np.sqrt(q.shape[-1])
    s = (q @ np.swapaxes(k, -1, -2)) * dtype(scale)
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    return (e / e.sum(axis=-1, keepdims=True)) @ v


def dot_exact(a, b):
    """a [..., M, K] . b [..., N, K]^T -> [..., M, N], every entry the correctly rounded sum (math.fsum) of its K rounded
    products: independent of the summation order and unchanged by zero terms, which is what the padded-head identity needs -
    a BLAS product blocks K = 72 and K = 128 differently."""
    prod = a[..., :, None, :] * b[..., None, :, :]
    return np.array([math.fsum(r) for r in prod.reshape(-1, prod.shape[-1])], prod.dtype).reshape(prod.shape[:-1])


def patchify(x, p: int):
    """[B, C, H, W] -> [B * hp * wp, C * p * p]: rows (h, w) row-major, columns (c, ph, pw)."""
    B, C, H, W = x.shape
    return x.reshape(B, C, H // p, p, W // p, p).transpose(0, 2, 4, 1, 3, 5).reshape(B * (H // p) * (W // p), C * p * p)


def unpatchify(x, B: int, Co: int, H: int, W: int, p: int):
    """[B * hp * wp, p * p * Co] with columns (ph, pw, c) -> [B, Co, H, W]."""
    return x.reshape(B, H // p, W // p, p, p, Co).transpose(0, 5, 1, 3, 2, 4).reshape(B, Co, H, W)


# ---- host tables: float64 arithmetic on float32 arguments, rounded to float32 once (as the reference's CPU paths evaluate) --------
def sinusoidal_timestep_embedding(timesteps, embedding_dim: int, max_period: float = 10000.0):
    """diffusion/ops: interleaved sin / cos, frequencies exp(-ln(max_period) * i / half_dim)."""
    t = np.asarray(timesteps, F32).reshape(-1).astype(np.float64)
    half = embedding_dim // 2
    freqs = np.exp(-np.log(np.float64(max_period)) * np.arange(half, dtype=np.float64) / half)
    args = t[:, None] * freqs[None, :]
    out = np.zeros((t.shape[0], embedding_dim), F32)
    out[:, 0:2 * half:2] = np.sin(args)
    out[:, 1:2 * half:2] = np.cos(args)
    return out


def model_sinusoidal_embedding(positions, dim: int):
    """models/dit: [sin | cos], frequencies exp(-i * ln(10000) / (half_dim - 1)); a zero column when dim is odd."""
    pos = np.asarray(positions, F32).reshape(-1).astype(np.float64)
    half = dim // 2
    freqs = np.exp(np.arange(half, dtype=np.float64) * -(np.log(np.float64(10000)) / (half - 1)))
    arg = pos[:, None] * freqs[None, :]
    out = np.concatenate([np.sin(arg), np.cos(arg)], axis=-1)
    if dim % 2:
        out = np.pad(out, ((0, 0), (0, 1)))
    return out.astype(F32)


def pos_embed_2d(embed_dim: int, grid_h: int, grid_w: int):
    """[grid_h * grid_w, embed_dim] = [height embedding | width embedding]; the grid is flattened COLUMN-major (h runs first),
    although the patch rows it is added to are row-major: the reference's behaviour, kept."""
    hh, ww = np.meshgrid(np.arange(grid_h, dtype=F32), np.arange(grid_w, dtype=F32), indexing="ij")
    return np.concatenate([model_sinusoidal_embedding(hh.flatten("F"), embed_dim // 2),
                           model_sinusoidal_embedding(ww.flatten("F"), embed_dim // 2)], axis=-1).astype(F32)


# ---- the model ------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Spec:
    hidden_size: int = 144
    num_layers: int = 2
    num_heads: int = 2
    in_channels: int = 4
    out_channels: int = 8
    patch_size: int = 2
    text_dim: int = 32
    ff_dim: int = 576
    geglu: bool = False


def fixture_spec() -> Spec:
    """The configuration tests/golden/g13_pixart.npz was recorded with: head_dim 72, a 3 x 5 patch grid at the fixture's latent."""
    return Spec()


FIXTURE_SEED = 1300
FIXTURE_LATENT = (2, 4, 6, 10)
FIXTURE_TEXT_TOKENS = 5
FIXTURE_TIMESTEP = 500.0
FIXTURE_TIMESTEPS = (500.0, 37.0)          # a second recording with one timestep per batch element
TIME_DIM = 256                             # width of the sinusoidal input of the timestep MLP


def keeps_float32(name: str) -> bool:
    """Weights the device holds in float32 whatever the model dtype: the patch embedding, the conditioning path and the
    modulation tables."""
    return name.startswith(("pos_embed.", "adaln_single.")) or name.endswith("scale_shift_table")


def make_weights(spec: Spec, seed: int) -> dict:
    """PixArt tensor names (the diffusers layout the reference reads).  Matrices at std 1 / sqrt(fan_in); biases and the
    modulation tables at std 0.3 - 0.5, so that every modulation vector and both batch elements move the output."""
    rng = np.random.default_rng(seed)
    D, p = spec.hidden_size, spec.patch_size
    w = {}

    def lin(name, n_out, n_in, bias_std=0.3):
        w[name + ".weight"] = (rng.standard_normal((n_out, n_in)) / np.sqrt(n_in)).astype(F32)
        w[name + ".bias"] = (bias_std * rng.standard_normal(n_out)).astype(F32)

    lin("pos_embed.proj", D, spec.in_channels * p * p)
    w["pos_embed.proj.weight"] = w["pos_embed.proj.weight"].reshape(D, spec.in_channels, p, p)
    lin("adaln_single.emb.timestep_embedder.linear_1", D, TIME_DIM)
    lin("adaln_single.emb.timestep_embedder.linear_2", D, D)
    lin("adaln_single.linear", 6 * D, D, bias_std=0.4)
    lin("caption_projection.linear_1", D, spec.text_dim)
    lin("caption_projection.linear_2", D, D)
    for i in range(spec.num_layers):
        b = f"transformer_blocks.{i}."
        w[b + "scale_shift_table"] = (0.5 * rng.standard_normal((6, D))).astype(F32)
        for attn in ("attn1", "attn2"):
            for proj in ("to_q", "to_k", "to_v", "to_out.0"):
                lin(b + f"{attn}.{proj}", D, D)
        lin(b + "ff.net.0.proj", spec.ff_dim * (2 if spec.geglu else 1), D)
        lin(b + "ff.net.2", D, spec.ff_dim)
    w["scale_shift_table"] = (0.5 * rng.standard_normal((2, D))).astype(F32)
    lin("proj_out", p * p * spec.out_channels, D)
    return w


def make_inputs(seed: int, spec: Spec | None = None, latent_shape=FIXTURE_LATENT, tokens: int = FIXTURE_TEXT_TOKENS):
    spec = spec or fixture_spec()
    rng = np.random.default_rng(seed + 1)
    latent = rng.standard_normal(latent_shape).astype(F32)
    text = rng.standard_normal((latent_shape[0], tokens, spec.text_dim)).astype(F32)
    return latent, text


def pad_heads(w2d, heads: int, head_dim: int, width: int, axis: int):
    """Spread `heads` groups of head_dim rows (axis 0) or columns (axis 1) to groups of `width`, zeros between."""
    w2d = np.asarray(w2d)
    shape = list(w2d.shape)
    shape[axis] = heads * width
    out = np.zeros(shape, w2d.dtype)
    for h in range(heads):
        src = [slice(None)] * w2d.ndim
        dst = [slice(None)] * w2d.ndim
        src[axis] = slice(h * head_dim, (h + 1) * head_dim)
        dst[axis] = slice(h * width, h * width + head_dim)
        out[tuple(dst)] = w2d[tuple(src)]
    return out


def gelu_tanh(x):
    dt = x.dtype.type
    return dt(0.5) * x * (1 + np.tanh(dt(np.sqrt(2 / np.pi)) * (x + dt(0.044715) * x ** 3)))


def silu(x):
    return x / (1 + np.exp(-x))


def forward(spec: Spec, weights: dict, latent, timestep, text, dtype=np.float64, round_dtype: str = "f32", head_width: int | None = None,
            swap_conditioning: bool = False, exact_sums: bool = False):
    """latent [B, C, H, W], timestep (scalar or [B]), text [B, M, text_dim] -> [B, out_channels, H, W] in `dtype`.
    round_dtype "bf16" / "f16": latent, text and every weight the device holds in 16 bits are rounded to it first.
    head_width: run attention on heads zero-padded to that width (the packed weights of the device model); the result equals the
    unpadded one exactly when exact_sums routes every product of the attention sub-layers through dot_exact (slow: for the
    fixture's shapes only).  swap_conditioning: batch element b is modulated by element B-1-b's conditioning - a wrong model, for
    negative controls."""
    w = {k: np.asarray(v if keeps_float32(k) else round_to(v, round_dtype), dtype) for k, v in weights.items()}
    latent = np.asarray(round_to(latent, round_dtype), dtype)
    text = np.asarray(round_to(text, round_dtype), dtype)
    B, C, H, W = latent.shape
    D, heads, p = spec.hidden_size, spec.num_heads, spec.patch_size
    hd = D // heads
    hp, wp = H // p, W // p
    N = hp * wp

    def lin(a, name):
        return a @ w[name + ".weight"].T + w[name + ".bias"]

    x = patchify(latent, p) @ w["pos_embed.proj.weight"].reshape(D, -1).T + w["pos_embed.proj.bias"]
    x = x.reshape(B, N, D) + np.asarray(pos_embed_2d(D, hp, wp), dtype)[None]
    t = np.broadcast_to(np.asarray(timestep, F32).reshape(-1), (B,))
    te = "adaln_single.emb.timestep_embedder."
    t_emb = lin(silu(lin(np.asarray(model_sinusoidal_embedding(t, TIME_DIM), dtype), te + "linear_1")), te + "linear_2")
    cond = lin(silu(t_emb), "adaln_single.linear").reshape(B, 6, D)
    if swap_conditioning:
        cond, t_emb = cond[::-1], t_emb[::-1]
    ctx = lin(silu(lin(text, "caption_projection.linear_1")), "caption_projection.linear_2")

    def mm(a, b_t):
        return dot_exact(a, b_t) if exact_sums else a @ np.swapaxes(b_t, -1, -2)

    def mha(xq, xkv, prefix):
        def heads_of(a, name):
            wt, bs = w[prefix + name + ".weight"], w[prefix + name + ".bias"]
            if head_width:
                wt, bs = pad_heads(wt, heads, hd, head_width, 0), pad_heads(bs, heads, hd, head_width, 0)
            return (mm(a, wt) + bs).reshape(B, a.shape[1], heads, -1).transpose(0, 2, 1, 3)

        q, k, v = heads_of(xq, "to_q"), heads_of(xkv, "to_k"), heads_of(xkv, "to_v")
        s = mm(q, k) * dtype(1.0 / np.sqrt(hd))
        e = np.exp(s - s.max(axis=-1, keepdims=True))
        o = mm(e / e.sum(axis=-1, keepdims=True), np.swapaxes(v, -1, -2))
        o = o.transpose(0, 2, 1, 3).reshape(B, xq.shape[1], -1)
        wo = w[prefix + "to_out.0.weight"]
        if head_width:
            wo = pad_heads(wo, heads, hd, head_width, 1)
        return mm(o, wo) + w[prefix + "to_out.0.bias"]

    for i in range(spec.num_layers):
        b = f"transformer_blocks.{i}."
        m = w[b + "scale_shift_table"][None] + cond                                     # [B, 6, D]
        shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp = (m[:, j][:, None, :] for j in range(6))
        h = layer_norm(x) * (1 + scale_msa) + shift_msa
        x = x + gate_msa * mha(h, h, b + "attn1.")
        x = x + mha(x, ctx, b + "attn2.")
        h = lin(layer_norm(x) * (1 + scale_mlp) + shift_mlp, b + "ff.net.0.proj")
        if w[b + "ff.net.0.proj.weight"].shape[0] == 2 * w[b + "ff.net.2.weight"].shape[1]:
            half = h.shape[-1] // 2
            h = gelu_tanh(h[..., :half]) * h[..., half:]
        else:
            h = gelu_tanh(h)
        x = x + gate_mlp * lin(h, b + "ff.net.2")
    tab = w["scale_shift_table"]
    x = layer_norm(x) * (1 + tab[1]) + (tab[0][None] + t_emb)[:, None, :]
    out = unpatchify(lin(x, "proj_out").reshape(B * N, -1), B, spec.out_channels, H, W, p)
    assert out.dtype == dtype
    return out
