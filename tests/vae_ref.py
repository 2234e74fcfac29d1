"""NumPy oracle of the VAE decoder path: conv2d as a direct sum, group_norm, and the AutoencoderKL decoder the SD / SDXL / SD3 /
Flux checkpoints hold (diffusers tensor names).  float64 by default; `dtype=np.float32` restates the same formulas in float32
(the yardstick of the float32 bars); `round_dtype` rounds weights and latent to a 16-bit format and `round_activations` rounds
every op's output as the device does (the floor of the 16-bit bars).  No torch, no device, no reference package."""

from __future__ import annotations

import numpy as np

from pygpukit_amd.diffusion.config import VAESpec

FIXTURE_SEED = 1414

# (N, C_in, C_out, H, W, K, stride, pad, dilation)
CONV_CASES = [
    (1, 32, 64, 8, 16, 3, 1, 1, 1),      # exact tile
    (2, 40, 70, 11, 19, 3, 1, 1, 1),     # every tail, two chunks, two patches each way, batch
    (1, 4, 3, 9, 17, 3, 1, 1, 1),        # tiny channel counts
    (1, 33, 64, 8, 16, 1, 1, 0, 1),      # 1x1
    (1, 8, 8, 17, 35, 3, 2, 1, 1),       # stride 2
    (1, 8, 8, 9, 9, 3, 1, 0, 1),         # no padding
    (1, 6, 5, 12, 10, 5, 1, 2, 1),       # 5x5: the FMA kernel in every dtype
    (1, 6, 5, 12, 10, 3, 1, 2, 2),       # dilation 2: the FMA kernel in every dtype
]
# what conv2d_plan promises for a 16-bit dtype (float32 is always "fma")
CONV_PLANS_16 = ["mfma", "mfma", "mfma", "mfma", "mfma", "mfma", "fma", "fma"]

# (N, C, H, W, G); (1, 32, 37, 31, 2): 16 channels per group -> 512-pixel chunks in the split plan, 1147 pixels = 2 chunks + 123;
# (2, 64, 40, 41, 16): 4 channels per group -> in 16-bit channels-last the split plan's row form, 1640 pixels = 3 chunks of 512 + 104;
# (1, 8, 5, 7, 8) and (2, 16, 6, 5, 8): 1 and 2 channels per group with C % 8 == 0 - the row form's other two instantiations
GN_CASES = [(2, 8, 3, 5, 2), (1, 6, 7, 9, 6), (1, 10, 4, 6, 2), (1, 32, 24, 40, 8), (1, 32, 37, 31, 2), (2, 64, 40, 41, 16),
            (1, 8, 5, 7, 8), (2, 16, 6, 5, 8)]
GN_STABLE_CASE = (1, 8, 24, 40, 2)       # inputs 100 + N(0, 1)


def conv_inputs(i: int):
    n, ci, co, h, w, k, s, p, d = CONV_CASES[i]
    rng = np.random.default_rng(FIXTURE_SEED + 100 + i)
    return (rng.standard_normal((n, ci, h, w)).astype(np.float32), (rng.standard_normal((co, ci, k, k)) / np.sqrt(ci * k * k)).astype(np.float32),
            rng.standard_normal(co).astype(np.float32))


def gn_inputs(i: int):
    n, c, h, w, g = GN_CASES[i]
    rng = np.random.default_rng(FIXTURE_SEED + 200 + i)
    return (rng.standard_normal((n, c, h, w)).astype(np.float32) * 2 + 0.5, (1 + 0.2 * rng.standard_normal(c)).astype(np.float32),
            (0.3 * rng.standard_normal(c)).astype(np.float32))


def gn_stable_inputs():
    """The stable-statistics case: x = 100 + N(0, 1) in float32 on GN_STABLE_CASE, gamma ~ 1 + 0.2 N, beta ~ 0.3 N."""
    n, c, h, w, _ = GN_STABLE_CASE
    rng = np.random.default_rng(77)
    x = (100.0 + rng.standard_normal((n, c, h, w))).astype(np.float32)
    return x, (1 + 0.2 * rng.standard_normal(c)).astype(np.float32), (0.3 * rng.standard_normal(c)).astype(np.float32)


# ------------------------------------------------------------------ rounding
def round_to(a: np.ndarray, name: "str | None") -> np.ndarray:
    """a rounded to nearest-even in `name` ("bfloat16" | "float16" | "float32" | None), returned in a's dtype."""
    if name is None or name == "float64":
        return a
    if name == "float32":
        return a.astype(np.float32).astype(a.dtype)
    if name == "float16":
        return a.astype(np.float16).astype(a.dtype)
    if name == "bfloat16":
        return _round_bf16(a).astype(a.dtype)
    raise ValueError(name)


def _round_bf16(a: np.ndarray) -> np.ndarray:
    """float64 -> nearest bfloat16 (8 significand bits, ties to even) in ONE rounding; normal range only"""
    m, e = np.frexp(np.asarray(a, np.float64))
    return np.ldexp(np.rint(m * 256.0) / 256.0, e)


# ------------------------------------------------------------------ ops
def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def upsample2(x: np.ndarray) -> np.ndarray:
    """nearest-neighbour 2x of [N, C, H, W]: out[y, x] = in[y >> 1, x >> 1]"""
    return np.repeat(np.repeat(x, 2, axis=2), 2, axis=3)


def conv2d(x, w, b=None, stride=1, padding=0, dilation=1, *, upsample=1, add=None, absolute=False, dtype=np.float64):
    """x [N, C_in, H, W], w [C_out, C_in, KH, KW], b [C_out] -> [N, C_out, Ho, Wo], a direct sum over the taps in `dtype`.
    absolute=True: sum |x| |w| + |b| (the magnitude the elementwise error bars scale with)."""
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    if absolute:
        x, w = np.abs(x), np.abs(w)
    if upsample == 2:
        x = upsample2(x)
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(padding), _pair(dilation)
    n, c, h, wd = x.shape
    m, c2, kh, kw = w.shape
    assert c == c2
    ho = (h + 2 * ph - (kh - 1) * dh - 1) // sh + 1
    wo = (wd + 2 * pw - (kw - 1) * dw - 1) // sw + 1
    xp = np.zeros((n, c, h + 2 * ph, wd + 2 * pw), dtype)
    xp[:, :, ph:ph + h, pw:pw + wd] = x
    out = np.zeros((n, m, ho, wo), dtype)
    for ky in range(kh):
        for kx in range(kw):
            win = xp[:, :, ky * dh: ky * dh + (ho - 1) * sh + 1: sh, kx * dw: kx * dw + (wo - 1) * sw + 1: sw]
            out += np.einsum("mc,nchw->nmhw", w[:, :, ky, kx], win, optimize=True).astype(dtype)
    if b is not None:
        bb = np.asarray(b, dtype)
        out += (np.abs(bb) if absolute else bb)[None, :, None, None]
    if add is not None:
        out += np.abs(np.asarray(add, dtype)) if absolute else np.asarray(add, dtype)
    return out


def group_norm(x, gamma, beta, groups, eps=1e-5, *, silu=False, dtype=np.float64):
    """x [N, C, H, W]; two-pass mean and population variance per (image, group) in `dtype`."""
    x = np.asarray(x, dtype)
    n, c, h, w = x.shape
    g = x.reshape(n, groups, -1)
    mean = g.mean(axis=2, keepdims=True, dtype=dtype)
    d = g - mean
    var = (d * d).mean(axis=2, keepdims=True, dtype=dtype)
    y = (d / np.sqrt(var + dtype(eps))).reshape(n, c, h, w)
    y = y * np.asarray(gamma, dtype)[None, :, None, None] + np.asarray(beta, dtype)[None, :, None, None]
    if silu:
        y = y / (1 + np.exp(-y))
    return y.astype(dtype)


def group_norm_one_pass(x, gamma, beta, groups, eps=1e-5, dtype=np.float32):
    """The formula a sum / sum-of-squares kernel computes: var = E[x^2] - E[x]^2 in `dtype`.  Only to show what test (c) pins."""
    x = np.asarray(x, dtype)
    n, c, h, w = x.shape
    g = x.reshape(n, groups, -1)
    cnt = dtype(g.shape[2])
    s1 = g.sum(axis=2, keepdims=True, dtype=dtype)
    s2 = (g * g).sum(axis=2, keepdims=True, dtype=dtype)
    mean = s1 / cnt
    var = np.maximum(s2 / cnt - mean * mean, dtype(0))
    y = ((g - mean) / np.sqrt(var + dtype(eps))).reshape(n, c, h, w)
    return (y * np.asarray(gamma, dtype)[None, :, None, None] + np.asarray(beta, dtype)[None, :, None, None]).astype(dtype)


# ------------------------------------------------------------------ decoder
def fixture_spec(shift_factor: float = 0.0) -> VAESpec:
    return VAESpec(name="fixture_vae", latent_channels=4, scaling_factor=0.5, block_out_channels=(16, 32, 32), layers_per_block=1,
                   norm_num_groups=4, norm_eps=1e-6, shift_factor=shift_factor)


def resnet_plan(spec) -> list:
    """[(prefix, c_in, c_out)] of every up-block resnet, and which blocks carry an upsampler: ([...], [bool])."""
    rc = list(reversed(spec.block_out_channels))
    res, ups, prev = [], [], rc[0]
    for i, ch in enumerate(rc):
        for j in range(spec.layers_per_block + 1):
            res.append((f"decoder.up_blocks.{i}.resnets.{j}.", i, prev if j == 0 else ch, ch))
        ups.append(i < len(rc) - 1)
        prev = ch
    return res, ups


def make_weights(spec, seed: int, post_quant: bool = True) -> dict:
    """float32 tensors under the diffusers names; convolutions ~ N(0, 1 / fan_in), norms gamma ~ 1 + 0.1 N, beta ~ 0.1 N."""
    rng = np.random.default_rng(seed)
    w = {}

    def conv(name, co, ci, k):
        w[name + ".weight"] = (rng.standard_normal((co, ci, k, k)) / np.sqrt(ci * k * k)).astype(np.float32)
        w[name + ".bias"] = (0.1 * rng.standard_normal(co)).astype(np.float32)

    def lin(name, co, ci):
        w[name + ".weight"] = (rng.standard_normal((co, ci)) / np.sqrt(ci)).astype(np.float32)
        w[name + ".bias"] = (0.1 * rng.standard_normal(co)).astype(np.float32)

    def norm(name, c):
        w[name + ".weight"] = (1 + 0.1 * rng.standard_normal(c)).astype(np.float32)
        w[name + ".bias"] = (0.1 * rng.standard_normal(c)).astype(np.float32)

    def resnet(p, ci, co):
        norm(p + "norm1", ci); conv(p + "conv1", co, ci, 3); norm(p + "norm2", co); conv(p + "conv2", co, co, 3)
        if ci != co:
            conv(p + "conv_shortcut", co, ci, 1)

    lc, top = spec.latent_channels, spec.block_out_channels[-1]
    if post_quant:
        conv("post_quant_conv", lc, lc, 1)
    conv("decoder.conv_in", top, lc, 3)
    resnet("decoder.mid_block.resnets.0.", top, top)
    a = "decoder.mid_block.attentions.0."
    norm(a + "group_norm", top)
    for n in ("to_q", "to_k", "to_v", "to_out.0"):
        lin(a + n, top, top)
    resnet("decoder.mid_block.resnets.1.", top, top)
    res, ups = resnet_plan(spec)
    for p, i, ci, co in res:
        resnet(p, ci, co)
    for i, up in enumerate(ups):
        if up:
            c = list(reversed(spec.block_out_channels))[i]
            conv(f"decoder.up_blocks.{i}.upsamplers.0.conv", c, c, 3)
    norm("decoder.conv_norm_out", spec.block_out_channels[0])
    conv("decoder.conv_out", spec.out_channels, spec.block_out_channels[0], 3)
    return w


def make_latent(seed: int, shape=(2, 4, 5, 7)) -> np.ndarray:
    return np.random.default_rng(seed + 1).standard_normal(shape).astype(np.float32)


def forward(spec, weights, latent, dtype=np.float64, round_dtype=None, round_activations=False, *, mutate=None):
    """decode(latent): x / scaling_factor + shift_factor, the decoder, the clamp to [-1, 1].  Weights and latent are rounded to
    `round_dtype` first; with round_activations every op's output is rounded to it too - one rounding per launch of the device
    decoder (a convolution with its residual add and its upsample is ONE op; so is group_norm + SiLU).
    mutate: a name of MUTATIONS, to prove that a wrong decoder lands far outside the bars."""
    W = {k: round_to(np.asarray(v, np.float64), round_dtype).astype(dtype) for k, v in weights.items()}
    r = (lambda a: round_to(a, round_dtype).astype(dtype)) if round_activations else (lambda a: a)
    G, eps = spec.norm_num_groups, spec.norm_eps

    def conv(x, name, pad, **kw):
        wt = W[name + ".weight"]
        if mutate == "dropped_tap" and wt.shape[2] == 3:
            wt = wt.copy()
            wt[:, :, 2, 2] = 0
        if mutate == "pad_off_by_one" and wt.shape[2] == 3:      # every tap reads one pixel up and left of where it should
            x = np.pad(x, ((0, 0), (0, 0), (1, 0), (1, 0)))[:, :, :-1, :-1]
        return r(conv2d(x, wt, W[name + ".bias"], 1, pad, dtype=dtype, **kw))

    def gn(x, name, silu):
        g = G
        if mutate == "group_shifted":
            xs = np.roll(x, 1, axis=1)
            y = group_norm(xs, np.roll(W[name + ".weight"], 1), np.roll(W[name + ".bias"], 1), g, eps, silu=silu, dtype=dtype)
            return r(np.roll(y, -1, axis=1))
        return r(group_norm(x, W[name + ".weight"], W[name + ".bias"], g, eps, silu=silu, dtype=dtype))

    def resnet(x, p):
        h = conv(gn(x, p + "norm1", True), p + "conv1", 1)
        sc = conv(x, p + "conv_shortcut", 0) if p + "conv_shortcut.weight" in W else x
        return conv(gn(h, p + "norm2", True), p + "conv2", 1, add=sc)

    def attention(x, p):
        n, c, h, w = x.shape
        rows = gn(x, p + "group_norm", False).transpose(0, 2, 3, 1).reshape(n, h * w, c)
        q, k, v = (r(rows @ W[p + t + ".weight"].reshape(c, c).T + W[p + t + ".bias"]) for t in ("to_q", "to_k", "to_v"))
        s = (q @ k.transpose(0, 2, 1)) / np.sqrt(dtype(c))
        s = np.exp(s - s.max(axis=2, keepdims=True))
        o = r((s / s.sum(axis=2, keepdims=True)) @ v)
        o = o @ W[p + "to_out.0.weight"].reshape(c, c).T + W[p + "to_out.0.bias"]
        return r(o.reshape(n, h, w, c).transpose(0, 3, 1, 2) + x)

    x = round_to(np.asarray(latent, np.float64), round_dtype).astype(dtype)
    x = r(x / dtype(spec.scaling_factor) + dtype(spec.shift_factor))
    if "post_quant_conv.weight" in W:
        x = conv(x, "post_quant_conv", 0)
    x = conv(x, "decoder.conv_in", 1)
    x = resnet(x, "decoder.mid_block.resnets.0.")
    x = attention(x, "decoder.mid_block.attentions.0.")
    x = resnet(x, "decoder.mid_block.resnets.1.")
    res, ups = resnet_plan(spec)
    for i, up in enumerate(ups):
        for p, bi, ci, co in res:
            if bi == i:
                x = resnet(x, p)
        if up:
            if mutate == "no_upsample_shift":
                # (y >> 1) replaced by y: reads the input at (y, x) clamped into range instead of (y >> 1, x >> 1)
                n, c, h, w = x.shape
                yy, xx = np.minimum(np.arange(2 * h), h - 1), np.minimum(np.arange(2 * w), w - 1)
                x = conv(x[:, :, yy][:, :, :, xx], f"decoder.up_blocks.{i}.upsamplers.0.conv", 1)
            else:
                x = conv(x, f"decoder.up_blocks.{i}.upsamplers.0.conv", 1, upsample=2)
    x = gn(x, "decoder.conv_norm_out", True)
    x = conv(x, "decoder.conv_out", 1)
    return np.clip(x, -1, 1)


MUTATIONS = ("dropped_tap", "pad_off_by_one", "group_shifted", "no_upsample_shift")


def rel_err(a, b) -> float:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
