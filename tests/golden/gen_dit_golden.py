"""Records tests/golden/g13_pixart.npz from the reference package's own CPU path (its CPU backend: no GPU, float32).

    python tests/golden/gen_dit_golden.py <path to the reference's src directory>

Only this generator imports the reference (`pygpukit`); the tests read the fixture.  The fixture stores inputs, the seed and
outputs; the weights are regenerated from tests/dit_ref.py's make_weights(fixture_spec(), seed).  Recorded:
  * latent [2, 4, 6, 10], text [2, 5, 32], timestep 500 -> out [2, 8, 6, 10]: the reference PixArtTransformer.forward on
    fixture_spec() (hidden 144, 2 heads of 72, 2 blocks, patch 2: a 3 x 5 grid, so the column-major position table is pinned);
  * out_t2: the same forward with one timestep per batch element (timesteps), so that the two elements are conditioned differently;
  * pos_embed, t_sin: the reference's get_2d_sincos_pos_embed(144, (3, 5)) and models/dit sinusoidal_embedding(timesteps, 256);
  * from diffusion/ops: ada_* (adaln and adaln_zero on [2, 5, 72] with [2, 72] vectors), ca_* (cross_attention, 4-D, q_len 7 !=
    kv_len 5), ts_* (sinusoidal_timestep_embedding at dims 64 and 10, the second with max_period 1000; the reference raises on an odd dim)."""

from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
from tests import dit_ref as R  # noqa: E402


def main(ref_src: str) -> None:
    sys.path.insert(0, ref_src)
    from pygpukit.core import from_numpy
    from pygpukit.diffusion.config import PixArtSpec
    from pygpukit.diffusion.models.dit.embeddings import get_2d_sincos_pos_embed, sinusoidal_embedding
    from pygpukit.diffusion.models.dit.model import PixArtTransformer
    from pygpukit.diffusion.ops import adaln, adaln_zero, cross_attention, sinusoidal_timestep_embedding

    spec = R.fixture_spec()
    rspec = PixArtSpec(name="fixture", hidden_size=spec.hidden_size, num_layers=spec.num_layers, num_heads=spec.num_heads,
                       conditioning_type="cross_attn", text_encoder_dim=spec.text_dim, pos_embed_type="sinusoidal",
                       patch_size=spec.patch_size, in_channels=spec.in_channels, out_channels=spec.out_channels,
                       cross_attention_dim=spec.text_dim)
    weights = R.make_weights(spec, R.FIXTURE_SEED)
    model = PixArtTransformer(rspec, {k: from_numpy(v) for k, v in weights.items()})
    latent, text = R.make_inputs(R.FIXTURE_SEED)
    rec = dict(seed=np.array(R.FIXTURE_SEED), latent=latent, text=text, timestep=np.array(R.FIXTURE_TIMESTEP, np.float32),
               timesteps=np.array(R.FIXTURE_TIMESTEPS, np.float32))
    rec["out"] = model.forward(from_numpy(latent), float(R.FIXTURE_TIMESTEP), from_numpy(text)).to_numpy()
    rec["out_t2"] = model.forward(from_numpy(latent), rec["timesteps"], from_numpy(text)).to_numpy()
    assert rec["out"].shape == (2, 8, 6, 10) and rec["out"].dtype == np.float32 and np.isfinite(rec["out"]).all()
    rec["pos_embed"] = get_2d_sincos_pos_embed(spec.hidden_size, (3, 5))
    rec["t_sin"] = sinusoidal_embedding(rec["timesteps"], R.TIME_DIM)

    rng = np.random.default_rng(R.FIXTURE_SEED + 2)
    x, res = (rng.standard_normal((2, 5, 72)).astype(np.float32) for _ in range(2))
    scale, shift, gate = (0.5 * rng.standard_normal((2, 72)).astype(np.float32) for _ in range(3))
    g = from_numpy
    rec.update(ada_x=x, ada_res=res, ada_scale=scale, ada_shift=shift, ada_gate=gate,
               ada_out=adaln(g(x), g(scale), g(shift)).to_numpy(),
               ada_zero_out=adaln_zero(g(x), g(scale), g(shift), g(gate), g(res)).to_numpy())
    q = rng.standard_normal((2, 3, 7, 16)).astype(np.float32)
    k, v = (rng.standard_normal((2, 3, 5, 16)).astype(np.float32) for _ in range(2))
    rec.update(ca_q=q, ca_k=k, ca_v=v, ca_out=cross_attention(g(q), g(k), g(v)).to_numpy())
    ts = np.array([0.0, 1.0, 37.0, 500.0, 999.0], np.float32)
    rec.update(ts_t=ts, ts_64=sinusoidal_timestep_embedding(ts, 64).to_numpy(),
               ts_10=sinusoidal_timestep_embedding(ts, 10, max_period=1000.0).to_numpy())

    path = os.path.join(HERE, "g13_pixart.npz")
    np.savez_compressed(path, **rec)
    print({k: v.shape for k, v in rec.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
