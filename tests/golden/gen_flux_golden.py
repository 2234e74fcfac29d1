"""Records tests/golden/g15_flux.npz from the reference package's own CPU path (its CPU backend: no GPU, float32).

    python tests/golden/gen_flux_golden.py <path to the reference's src directory>

Only this generator imports the reference (`pygpukit`); the tests read the fixture.  The fixture stores inputs, the seed and
outputs; the weights are regenerated from tests/flux_ref.py's make_weights(fixture_config(), seed).

The reference's CPU backend cannot add a bias: ops.nn.linear._bias_add_inplace_cpu assigns `output._data`, which a GPUArray does
not have, so gpu_linear fails on the first biased layer.  This generator therefore rebinds the name `bias_add_inplace` in the
reference's models.flux.ops module to a few lines of its own, which give the array the device pointer of a fresh array holding
y + b (the temporary is kept alive).  With that gpu_linear is x @ W.T + b and FluxTransformer.forward runs on the CPU.

Recorded:
  * hidden [2, 6, 8], text [2, 5, 24], pooled [2, 12], ids; out (timestep 750 for both elements), out_t2 (timesteps 750, 250):
    FluxTransformer.forward on fixture_config() (hidden 128, 2 heads of 64, axes (16, 24, 24), 2 double + 2 single blocks);
  * out_guid: a guidance_embeds=True weight set (seed + 10) with guidance (3.5, 1.5);
  * rope_cos / rope_sin, img_ids / txt_ids, t_emb: get_rope_frequencies, prepare_*_ids, timestep_embedding(timesteps, 256);
  * ja_* / sa_out: stand-alone joint_attention and single_attention on flux_ref.make_attention_case(seed + 3) (outputs and the
    RoPE tables only; the case is regenerated from the seed);
  * nr_*: gpu_rms_norm per head then apply_rope on [2, 11, 3, 64] with a random general table;
  * sched_*: sigmas / timesteps for (4 steps, shift 1), (5 steps, shift 3), dynamic shifting at 256 and 4096 image tokens, and a
    4-step `step` trajectory;
  * unpack_in / unpack_out: FluxPipeline._unpack_latents of [2, 6, 64] at height 32, width 48."""

from __future__ import annotations

import dataclasses
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
from tests import flux_ref as R  # noqa: E402


def main(ref_src: str) -> None:
    sys.path.insert(0, ref_src)
    from pygpukit.core.factory import from_numpy
    from pygpukit.diffusion.models.flux import ops as flux_ops

    keep = []

    def bias_add_inplace(y, b):
        t = from_numpy(y.to_numpy() + b.to_numpy())
        keep.append(t)
        y._device_ptr = t._device_ptr

    flux_ops.bias_add_inplace = bias_add_inplace
    from pygpukit.diffusion.models.flux import attention as A
    from pygpukit.diffusion.models.flux.embeddings import (apply_rope, get_rope_frequencies, prepare_image_ids, prepare_text_ids,
                                                           timestep_embedding)
    from pygpukit.diffusion.models.flux.model import FluxConfig, FluxTransformer
    from pygpukit.diffusion.models.flux.pipeline import FluxPipeline
    from pygpukit.diffusion.models.flux.scheduler import FlowMatchEulerScheduler, FlowMatchEulerSchedulerConfig

    g = from_numpy
    x = g(np.arange(6, dtype=np.float32).reshape(2, 3))
    w, b = np.arange(12, dtype=np.float32).reshape(4, 3) / 7, np.arange(4, dtype=np.float32)
    assert np.array_equal(flux_ops.gpu_linear(x, g(w), g(b)).to_numpy(), x.to_numpy() @ w.T + b), "the patched gpu_linear"

    cfg = R.fixture_config()

    def model_for(c: R.Config, seed: int):
        rc = FluxConfig(in_channels=c.in_channels, hidden_size=c.hidden_size, num_layers=c.num_layers,
                        num_single_layers=c.num_single_layers, num_attention_heads=c.num_attention_heads,
                        attention_head_dim=c.attention_head_dim, joint_attention_dim=c.joint_attention_dim,
                        pooled_projection_dim=c.pooled_projection_dim, guidance_embeds=c.guidance_embeds, axes_dims_rope=c.axes_dims_rope)
        return FluxTransformer(rc, {k: g(v) for k, v in R.make_weights(c, seed).items()})

    hidden, text, pooled = R.make_inputs(R.FIXTURE_SEED)
    B, T = hidden.shape[0], text.shape[1]
    img_ids, txt_ids = prepare_image_ids(B, *R.FIXTURE_GRID), prepare_text_ids(B, T)
    ts = np.array(R.FIXTURE_TIMESTEPS, np.float32)
    rec = dict(seed=np.array(R.FIXTURE_SEED), hidden=hidden, text=text, pooled=pooled, img_ids=img_ids, txt_ids=txt_ids,
               timestep=np.array(R.FIXTURE_TIMESTEP, np.float32), timesteps=ts, guidance=np.array(R.FIXTURE_GUIDANCE, np.float32))

    def run(model, t, guidance=None):
        out = model.forward(g(hidden), g(text), g(pooled), t, img_ids=img_ids, txt_ids=txt_ids, guidance=guidance).to_numpy()
        assert out.shape == hidden.shape and out.dtype == np.float32 and np.isfinite(out).all()
        return out

    model = model_for(cfg, R.FIXTURE_SEED)
    rec["out"] = run(model, np.full(B, R.FIXTURE_TIMESTEP, np.float32))
    rec["out_t2"] = run(model, ts)
    rec["out_guid"] = run(model_for(dataclasses.replace(cfg, guidance_embeds=True), R.FIXTURE_SEED + 10), ts, rec["guidance"])
    rec["rope_cos"], rec["rope_sin"] = get_rope_frequencies(img_ids[0], txt_ids[0], axes_dim=cfg.axes_dims_rope)
    rec["t_emb"] = timestep_embedding(ts, 256)

    # stand-alone attention: D = 128 = 2 heads of 64, 3 text + 4 image tokens
    rng = np.random.default_rng(R.FIXTURE_SEED + 2)
    H, hd, Tt = 2, 64, 3
    ja = R.make_attention_case(R.FIXTURE_SEED + 3)
    ja["cos"], ja["sin"] = get_rope_frequencies(prepare_image_ids(1, 2, 2)[0], prepare_text_ids(1, Tt)[0], axes_dim=cfg.axes_dims_rope)
    o_img, o_txt = A.joint_attention(g(ja["img"]), g(ja["txt"]), g(ja["q"]), g(ja["k"]), g(ja["v"]), g(ja["q_b"]), g(ja["k_b"]), g(ja["v_b"]),
                                     g(ja["add_q"]), g(ja["add_k"]), g(ja["add_v"]), g(ja["add_q_b"]), g(ja["add_k_b"]), g(ja["add_v_b"]),
                                     g(ja["out"]), g(ja["out_b"]), g(ja["add_out"]), g(ja["add_out_b"]), g(ja["norm_q"]), g(ja["norm_k"]),
                                     g(ja["norm_added_q"]), g(ja["norm_added_k"]), g(ja["cos"]), g(ja["sin"]), num_heads=H, head_dim=hd)
    rec.update(ja_cos=ja["cos"], ja_sin=ja["sin"], ja_out_img=o_img.to_numpy(), ja_out_txt=o_txt.to_numpy())
    joint = np.concatenate([ja["txt"], ja["img"]], axis=1)
    rec["sa_out"] = A.single_attention(g(joint), g(ja["q"]), g(ja["k"]), g(ja["v"]), g(ja["q_b"]), g(ja["k_b"]), g(ja["v_b"]), g(ja["norm_q"]),
                                       g(ja["norm_k"]), g(ja["cos"]), g(ja["sin"]), num_heads=H, head_dim=hd).to_numpy()

    nr_x = rng.standard_normal((2, 11, 3, 64)).astype(np.float32)
    nr_w = (1 + 0.3 * rng.standard_normal(64)).astype(np.float32)
    nr_cos, nr_sin = (rng.uniform(-1, 1, (11, 64)).astype(np.float32) for _ in range(2))
    rec.update(nr_x=nr_x, nr_w=nr_w, nr_cos=nr_cos, nr_sin=nr_sin,
               nr_out=apply_rope(flux_ops.gpu_rms_norm(g(nr_x), g(nr_w)).to_numpy(), nr_cos, nr_sin).astype(np.float32))

    def sched(steps, mu_len=None, **kw):
        s = FlowMatchEulerScheduler(FlowMatchEulerSchedulerConfig(**kw))
        s.set_timesteps(steps, mu=None if mu_len is None else s.compute_mu(mu_len))
        return s

    for name, s in (("4_1", sched(4)), ("5_3", sched(5, shift=3.0)), ("dyn256", sched(4, 256, use_dynamic_shifting=True)),
                    ("dyn4096", sched(4, 4096, use_dynamic_shifting=True))):
        rec["sched_sigmas_" + name], rec["sched_timesteps_" + name] = s.sigmas, s.timesteps
    rec["sched_mu"] = np.array([sched(1).compute_mu(n) for n in (256, 1024, 4096)], np.float64)
    s = sched(4)
    sample = rng.standard_normal((2, 6, 8)).astype(np.float32)
    vel = rng.standard_normal((4, 2, 6, 8)).astype(np.float32)
    traj = [sample]
    for i, t in enumerate(s.timesteps):
        traj.append(s.step(vel[i], t, traj[-1]))
    rec.update(sched_sample=sample, sched_velocity=vel, sched_trajectory=np.stack(traj[1:]))

    unpack_in = rng.standard_normal((2, 6, 64)).astype(np.float32)
    rec.update(unpack_in=unpack_in, unpack_out=np.ascontiguousarray(FluxPipeline._unpack_latents(None, unpack_in, 32, 48)))

    path = os.path.join(HERE, "g15_flux.npz")
    np.savez_compressed(path, **rec)
    print({k: v.shape for k, v in rec.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
