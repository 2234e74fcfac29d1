"""Time the VAE decoder path (conv2d, group_norm, the mid-block attention, VAE.decode) in one process with alternating windows:
per round every variant of a line once, then the first variant again (A'), N calls each between device events after a warm-up of
all of them.  Prints the median us per call, the ratios, and the spread of the first variant against itself (A' / A: the margin
inside which two numbers are "the same").  Not a pass / fail gate.  All activations channels-last, weights packed, as the model.

  (a) conv2d 3x3 in bfloat16 at the decoder's four stages (512->512 at 128^2 and 256^2, 256->256 at 512^2, 128->128 at 1024^2):
      TFLOP/s and the ratio to matmul_nt at equal M x N x K (pixels x C_out x 9 C_in) in the same run; then 128->3 (conv_out) and
      4->512 (conv_in), where padding to the 64 x 32 tile wastes most of it, on the MFMA and on the FMA kernel;
  (b) fused against separate launches: upsample=2 against the convolution of a pre-upsampled tensor plus a device copy of that
      tensor (the least an upsample launch would move; the project has no upsample op); add= against conv2d + add;
      group_norm_silu against group_norm + silu;
  (c) the two group_norm plans at each stage in TB/s of the bytes that must move (one read and one write of the tensor);
  (d) the two attention paths (C = 512, one head) at 64, 256, 1024, 4096 and 16384 tokens (the first three ground vae_plan's
      threshold); the fallback kernel stops at 15360 keys;
  (e) a whole decode at 64^2 and 128^2 latents, SDXL spec, synthetic weights, float32 and bfloat16.

  --tile: section (a)'s four stages with the MFMA kernel's patch forced to 8 x 16 and to 16 x 16 pixels (PGK_CONV2D_ROWS), the
  measurement behind the tile rule in ops_conv2d.hip.

usage: vae_bench.py [--rounds N] [--out FILE] [--sections abcde] [--tile]"""
import argparse, ctypes as C, os, statistics, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from pygpukit_amd import _hip
from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import as_dtype, bfloat16, float32
from pygpukit_amd.core.factory import from_numpy

LINES = []
STAGES = [(512, 128), (512, 256), (256, 512), (128, 1024)]       # (channels, side) of the decoder's four stages at a 128^2 latent


def say(s=""):
    print(s, flush=True); LINES.append(s)


def rnd(shape, dt=bfloat16, seed=0, std=1.0):
    a = np.random.default_rng(seed).standard_normal(int(np.prod(shape)), dtype=np.float32).reshape(shape) * np.float32(std)
    return from_numpy(a).astype(dt)


class Timer:
    def __init__(self):
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        _hip.call("pgk_event_create", C.byref(self.e0)); _hip.call("pgk_event_create", C.byref(self.e1))

    def window_us(self, run, n):
        _hip.call("pgk_event_record", self.e0, None)
        for _ in range(n): run()
        _hip.call("pgk_event_record", self.e1, None); _hip.call("pgk_event_sync", self.e1)
        ms = C.c_float(); _hip.call("pgk_event_elapsed_ms", self.e0, self.e1, C.byref(ms))
        return ms.value * 1000 / n


def measure(timer, variants, rounds, n):
    """-> ({name: median us}, A' / A of the first variant)."""
    names = list(variants)
    for k in names: variants[k]()
    _hip.call("pgk_device_sync")
    t, again = {k: [] for k in names}, []
    for _ in range(rounds):
        for k in names: t[k].append(timer.window_us(variants[k], n))
        again.append(timer.window_us(variants[names[0]], n))
    med = {k: statistics.median(v) for k, v in t.items()}
    return med, statistics.median(again) / med[names[0]]


def with_env(name, value, fn):
    def run():
        old = os.environ.get(name)
        os.environ[name] = value
        try:
            fn()
        finally:
            if old is None: del os.environ[name]
            else: os.environ[name] = old
    return run


def section_a(timer, rounds):
    from pygpukit_amd.ops.conv import conv2d, conv2d_pack_weight, conv2d_plan
    from pygpukit_amd.ops.matmul import matmul_nt

    say("(a) conv2d 3x3, stride 1, padding 1, bfloat16, channels-last in and out, packed weight")
    for c, side in STAGES:
        x, w, b = rnd((1, side, side, c)), rnd((c, c, 3, 3), std=0.02, seed=1), rnd((c,), seed=2)
        pw, out = conv2d_pack_weight(w), GPUArray((1, side, side, c), bfloat16)
        M, N, K = side * side, c, 9 * c
        ga, gw, gout = rnd((M, K), seed=3), rnd((N, K), std=0.02, seed=4), GPUArray((M, N), bfloat16)
        med, aa = measure(timer, {"conv": lambda: conv2d(x, w, b, 1, 1, channels_last=True, channels_last_out=True, packed_weight=pw, out=out),
                                  "gemm": lambda: matmul_nt(ga, gw, b, out=gout)}, rounds, 3)
        fl = 2.0 * M * N * K
        say(f"  {c}->{c} at {side}^2 [{conv2d_plan(c, c, side, side, 3, 1, 1, 1, bfloat16)}]: {med['conv']:9.1f} us {fl / med['conv'] / 1e6:7.1f} TFLOP/s | "
            f"matmul_nt {M}x{N}x{K}: {med['gemm']:9.1f} us {fl / med['gemm'] / 1e6:7.1f} TFLOP/s | conv/gemm time {med['conv'] / med['gemm']:.2f} | A'/A {aa:.3f}")
        del ga, gw, gout
    for ci, co, side in ((128, 3, 512), (4, 512, 128)):
        x, w, b = rnd((1, side, side, ci)), rnd((co, ci, 3, 3), std=0.05, seed=1), rnd((co,), seed=2)
        pw, out = conv2d_pack_weight(w), GPUArray((1, side, side, co), bfloat16)
        run = lambda: conv2d(x, w, b, 1, 1, channels_last=True, channels_last_out=True, packed_weight=pw, out=out)   # noqa: E731
        med, aa = measure(timer, {"mfma": run, "fma": with_env("PGK_CONV_MFMA", "0", run)}, rounds, 3)
        fl = 2.0 * side * side * co * 9 * ci
        say(f"  {ci}->{co} at {side}^2: mfma {med['mfma']:9.1f} us {fl / med['mfma'] / 1e6:6.2f} TFLOP/s | fma {med['fma']:9.1f} us "
            f"{fl / med['fma'] / 1e6:6.2f} TFLOP/s | fma/mfma {med['fma'] / med['mfma']:.2f} | A'/A {aa:.3f}")


def section_tile(timer, rounds):
    from pygpukit_amd.ops.conv import conv2d, conv2d_pack_weight

    say("(tile) conv2d 3x3 bfloat16 channels-last, patch rows forced: 8 x 16 against 16 x 16 pixels per workgroup")
    for c, side in STAGES:
        x, w, b = rnd((1, side, side, c)), rnd((c, c, 3, 3), std=0.02, seed=1), rnd((c,), seed=2)
        pw, out = conv2d_pack_weight(w), GPUArray((1, side, side, c), bfloat16)
        run = lambda: conv2d(x, w, b, 1, 1, channels_last=True, channels_last_out=True, packed_weight=pw, out=out)   # noqa: E731
        med, aa = measure(timer, {"8": with_env("PGK_CONV2D_ROWS", "8", run), "16": with_env("PGK_CONV2D_ROWS", "16", run)}, rounds, 3)
        fl = 2.0 * side * side * c * 9 * c
        say(f"  {c}->{c} at {side}^2: 8 rows {med['8']:9.1f} us {fl / med['8'] / 1e6:7.1f} TFLOP/s | 16 rows {med['16']:9.1f} us "
            f"{fl / med['16'] / 1e6:7.1f} TFLOP/s | 8/16 time {med['8'] / med['16']:.2f} | A'/A {aa:.3f}")


def section_b(timer, rounds):
    from pygpukit_amd.ops.conv import conv2d, conv2d_pack_weight
    from pygpukit_amd.ops.elementwise import add, copy_to
    from pygpukit_amd.ops.nn.activation import silu
    from pygpukit_amd.ops.nn.norm import group_norm, group_norm_silu

    say("(b) fused against separate launches, bfloat16, channels-last")
    c, side = 512, 128
    x, w, b = rnd((1, side, side, c)), rnd((c, c, 3, 3), std=0.02, seed=1), rnd((c,), seed=2)
    pw = conv2d_pack_weight(w)
    up, up2 = rnd((1, 2 * side, 2 * side, c), seed=5), GPUArray((1, 2 * side, 2 * side, c), bfloat16)
    out = GPUArray((1, 2 * side, 2 * side, c), bfloat16)
    kw = dict(channels_last=True, channels_last_out=True, packed_weight=pw)

    def separate():
        copy_to(up, up2)
        conv2d(up2, w, b, 1, 1, out=out, **kw)
    med, aa = measure(timer, {"fused": lambda: conv2d(x, w, b, 1, 1, upsample=2, out=out, **kw), "separate": separate}, rounds, 3)
    say(f"  upsample 2x + conv 512->512, {side}^2 -> {2 * side}^2: fused {med['fused']:9.1f} us | copy + conv {med['separate']:9.1f} us | "
        f"separate/fused {med['separate'] / med['fused']:.2f} | A'/A {aa:.3f}")
    res, o1 = rnd((1, side, side, c), seed=6), GPUArray((1, side, side, c), bfloat16)

    def sep_add():
        conv2d(x, w, b, 1, 1, out=o1, **kw)
        add(o1, res, out=o1)
    med, aa = measure(timer, {"fused": lambda: conv2d(x, w, b, 1, 1, add=res, out=o1, **kw), "separate": sep_add}, rounds, 5)
    say(f"  conv 512->512 at {side}^2 + residual: add= {med['fused']:9.1f} us | conv + add {med['separate']:9.1f} us | "
        f"separate/fused {med['separate'] / med['fused']:.2f} | A'/A {aa:.3f}")
    for c, side in STAGES:
        x, g, bt = rnd((1, side, side, c)), rnd((c,), seed=1), rnd((c,), seed=2)
        y = GPUArray((1, side, side, c), bfloat16)

        def sep_silu():
            group_norm(x, g, bt, 32, 1e-6, channels_last=True, out=y)
            silu(y, out=y)
        med, aa = measure(timer, {"fused": lambda: group_norm_silu(x, g, bt, 32, 1e-6, channels_last=True, out=y), "separate": sep_silu}, rounds, 5)
        say(f"  group_norm_silu {c} ch at {side}^2: fused {med['fused']:9.1f} us | group_norm + silu {med['separate']:9.1f} us | "
            f"separate/fused {med['separate'] / med['fused']:.2f} | A'/A {aa:.3f}")


def section_c(timer, rounds):
    from pygpukit_amd.ops.nn.norm import group_norm_plan, group_norm_silu

    say("(c) group_norm_silu plans, bfloat16, channels-last, 32 groups; TB/s of one read + one write of the tensor")
    for c, side in STAGES:
        x, g, bt = rnd((1, side, side, c)), rnd((c,), seed=1), rnd((c,), seed=2)
        y = GPUArray((1, side, side, c), bfloat16)
        run = lambda: group_norm_silu(x, g, bt, 32, 1e-6, channels_last=True, out=y)   # noqa: E731
        med, aa = measure(timer, {"split": with_env("PGK_GN_SPLIT", "1", run), "block": with_env("PGK_GN_SPLIT", "0", run)}, rounds, 3)
        by = 2.0 * side * side * c * 2
        say(f"  {c} ch at {side}^2 (group {c // 32} x {side * side}) [{group_norm_plan(1, c, side * side, 32, bfloat16, True)}]: "
            f"split {med['split']:9.1f} us {by / med['split'] / 1e6:5.2f} TB/s | block {med['block']:9.1f} us {by / med['block'] / 1e6:5.2f} TB/s | A'/A {aa:.3f}")


def section_d(timer, rounds):
    from tests import vae_ref as R
    from pygpukit_amd.diffusion import VAE, VAESpec

    say("(d) mid-block attention, C = 512, one head, one image: group_norm, projections, attention, out projection, residual")
    spec = VAESpec(name="attn", latent_channels=4, block_out_channels=(32, 512), layers_per_block=0, norm_num_groups=32)
    weights = R.make_weights(spec, 3)
    for dt in ("bfloat16", "float32"):
        vae = {p: VAE(spec, weights, dtype=dt, attention=p) for p in ("matmul", "sdpa")}
        for side in (8, 16, 32, 64, 128):
            x = rnd((1, side, side, 512), as_dtype(dt))
            variants = {"matmul": lambda: vae["matmul"]._attention(x, "matmul")}
            if side * side <= 15360:
                variants["sdpa"] = lambda: vae["sdpa"]._attention(x, "sdpa")
            med, aa = measure(timer, variants, max(2, rounds // 2) if side >= 64 else rounds, 1 if side >= 64 else 5)
            s = f"sdpa {med['sdpa']:11.1f} us | sdpa/matmul {med['sdpa'] / med['matmul']:.1f}" if "sdpa" in med else "sdpa: the fallback kernel stops at 15360 keys"
            say(f"  {dt} {side * side} tokens: matmul {med['matmul']:11.1f} us (scores {side ** 4 * as_dtype(dt).itemsize / 2 ** 20:.0f} MiB) | {s} | A'/A {aa:.3f}")


def section_e(timer, rounds):
    from tests import vae_ref as R
    from pygpukit_amd.diffusion import SDXL_VAE_SPEC, VAE, vae_plan

    say("(e) VAE.decode, SDXL spec, synthetic weights, batch 1")
    weights = R.make_weights(SDXL_VAE_SPEC, 5)
    for dt in ("bfloat16", "float32"):
        vae = VAE(SDXL_VAE_SPEC, weights, dtype=dt)
        for side in (64, 128):
            lat = rnd((1, 4, side, side), as_dtype(dt))
            plan = vae_plan(SDXL_VAE_SPEC, dt, (side, side))
            med, aa = measure(timer, {"decode": lambda: vae.decode(lat)}, max(2, rounds // 2), 1)
            say(f"  {dt} latent {side}^2 -> {8 * side}^2: {med['decode'] / 1000:9.2f} ms | {plan['launches']} launches, attention {plan['attention']}, "
                f"conv {plan['conv']}, group_norm {plan['group_norm']} | A'/A {aa:.3f}")
        del vae


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sections", default="abcde")
    ap.add_argument("--tile", action="store_true")
    a = ap.parse_args()
    props = _hip.DeviceProps()
    _hip.load().pgk_device_props(0, C.byref(props))
    say(f"vae_bench on {props.name.decode()} ({props.arch.decode()}), {a.rounds} rounds, median us per call")
    timer = Timer()
    for s, fn in (("a", section_a), ("b", section_b), ("c", section_c), ("d", section_d), ("e", section_e)):
        if s in a.sections:
            fn(timer, a.rounds)
    if a.tile:
        section_tile(timer, a.rounds)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
