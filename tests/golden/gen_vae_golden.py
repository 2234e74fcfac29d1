"""Records tests/golden/g14_vae.npz.

    python tests/golden/gen_vae_golden.py <path to the reference's src directory>

Only this generator imports the reference (`pygpukit`) and torch; the tests read the fixture.  Inputs are regenerated from
tests/vae_ref.py (case lists, make_weights, make_latent and the seeds recorded here).  Recorded:
  * conv_<i>: the reference's CPU conv2d (diffusion/ops/conv2d.py, float32) on CONV_CASES[i] for i in REF_CONV;
  * gn_<i>, gns_<i>: the reference's CPU group_norm and group_norm_silu on GN_CASES[i] for i in REF_GN;
  * tconv_<i>, tgn_<i>: torch float64 F.conv2d on CONV_CASES[i] for i in TORCH_CONV, F.group_norm on GN_CASES[i] for i in TORCH_GN;
  * dec, dec_nopq, dec_shift: the decoder on fixture_spec() restated in torch float64 - F.conv2d, F.group_norm, F.silu,
    F.interpolate(mode="nearest"), F.scaled_dot_product_attention - with post_quant_conv, without it, and with shift_factor
    0.25 (the reference has no decoder to record: its _decoder_forward_full is conv_in followed by scipy's zoom)."""

from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
from tests import vae_ref as R  # noqa: E402

REF_CONV = (1, 3, 4, 7)
REF_GN = (0, 1, 2)
TORCH_CONV = (2, 3, 4, 5, 6, 7)     # the small ones: the fixture stays far below the size limit
TORCH_GN = (0, 1, 2)
SHIFT = 0.25


def torch_decoder(spec, weights, latent):
    import torch
    import torch.nn.functional as F

    W = {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in weights.items()}
    G, eps = spec.norm_num_groups, spec.norm_eps

    def conv(x, name, pad):
        return F.conv2d(x, W[name + ".weight"], W[name + ".bias"], padding=pad)

    def gn(x, name):
        return F.group_norm(x, G, W[name + ".weight"], W[name + ".bias"], eps)

    def resnet(x, p):
        h = conv(F.silu(gn(x, p + "norm1")), p + "conv1", 1)
        h = conv(F.silu(gn(h, p + "norm2")), p + "conv2", 1)
        return h + (conv(x, p + "conv_shortcut", 0) if p + "conv_shortcut.weight" in W else x)

    def attention(x, p):
        n, c, h, w = x.shape
        rows = gn(x, p + "group_norm").permute(0, 2, 3, 1).reshape(n, h * w, c)
        q, k, v = (F.linear(rows, W[p + t + ".weight"], W[p + t + ".bias"]) for t in ("to_q", "to_k", "to_v"))
        o = F.scaled_dot_product_attention(q[:, None], k[:, None], v[:, None])[:, 0]
        o = F.linear(o, W[p + "to_out.0.weight"], W[p + "to_out.0.bias"])
        return o.reshape(n, h, w, c).permute(0, 3, 1, 2) + x

    x = torch.from_numpy(np.asarray(latent, np.float64)) / spec.scaling_factor + spec.shift_factor
    if "post_quant_conv.weight" in W:
        x = conv(x, "post_quant_conv", 0)
    x = conv(x, "decoder.conv_in", 1)
    x = resnet(x, "decoder.mid_block.resnets.0.")
    x = attention(x, "decoder.mid_block.attentions.0.")
    x = resnet(x, "decoder.mid_block.resnets.1.")
    n_blocks = len(spec.block_out_channels)
    for i in range(n_blocks):
        for j in range(spec.layers_per_block + 1):
            x = resnet(x, f"decoder.up_blocks.{i}.resnets.{j}.")
        if i < n_blocks - 1:
            x = conv(F.interpolate(x, scale_factor=2.0, mode="nearest"), f"decoder.up_blocks.{i}.upsamplers.0.conv", 1)
    x = conv(F.silu(gn(x, "decoder.conv_norm_out")), "decoder.conv_out", 1)
    return x.clamp(-1, 1).numpy()


def main(ref_src: str) -> None:
    import torch
    import torch.nn.functional as F

    sys.path.insert(0, ref_src)
    from pygpukit.core import from_numpy
    from pygpukit.diffusion.ops.conv2d import conv2d
    from pygpukit.diffusion.ops.group_norm import group_norm, group_norm_silu

    g = from_numpy
    rec = dict(seed=np.array(R.FIXTURE_SEED), ref_conv=np.array(REF_CONV), ref_gn=np.array(REF_GN), torch_conv=np.array(TORCH_CONV), torch_gn=np.array(TORCH_GN), shift=np.array(SHIFT))
    for i, case in enumerate(R.CONV_CASES):
        x, w, b = R.conv_inputs(i)
        s, p, d = case[6:9]
        if i in REF_CONV:
            rec[f"conv_{i}"] = conv2d(g(x), g(w), g(b), stride=s, padding=p, dilation=d).to_numpy()
        t = torch.from_numpy
        if i in TORCH_CONV:
            rec[f"tconv_{i}"] = F.conv2d(t(x).double(), t(w).double(), t(b).double(), stride=s, padding=p, dilation=d).numpy()
    for i, case in enumerate(R.GN_CASES):
        x, gamma, beta = R.gn_inputs(i)
        if i in REF_GN:
            rec[f"gn_{i}"] = group_norm(g(x), g(gamma), g(beta), case[4], 1e-5).to_numpy()
            rec[f"gns_{i}"] = group_norm_silu(g(x), g(gamma), g(beta), case[4], 1e-5).to_numpy()
        t = torch.from_numpy
        if i in TORCH_GN:
            rec[f"tgn_{i}"] = F.group_norm(t(x).double(), case[4], t(gamma).double(), t(beta).double(), 1e-5).numpy()
    latent = R.make_latent(R.FIXTURE_SEED)
    spec = R.fixture_spec()
    rec["dec"] = torch_decoder(spec, R.make_weights(spec, R.FIXTURE_SEED), latent)
    rec["dec_nopq"] = torch_decoder(spec, R.make_weights(spec, R.FIXTURE_SEED, post_quant=False), latent)
    rec["dec_shift"] = torch_decoder(R.fixture_spec(SHIFT), R.make_weights(spec, R.FIXTURE_SEED), latent)
    assert rec["dec"].shape == (2, 3, 20, 28) and np.isfinite(rec["dec"]).all()
    out = os.path.join(HERE, "g14_vae.npz")
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
