"""Time the diffusion-transformer path at PixArt-Sigma's shape (hidden 1152, 16 heads of 72, 28 blocks, 4096 tokens = 1024 px,
300 text tokens of 4096 features), all in bfloat16, in one process with alternating windows: per round every variant of a
section once, then the first variant again (A'), N calls each between device events after a warm-up of all of them.  Prints
the median us per call, the ratios, and the spread of the first variant against itself (A' / A: the margin inside which two
numbers are "the same").  Not a pass / fail gate.

  (a) the fused row kernel (diffusion.ops) against the composition of the existing ops (mul / add / layernorm with a ones /
      zeros gamma / beta, on [B N, D] broadcasts made on the host beforehand and not timed) at [2, 4096, 1152], for the three
      positions of a block, with the achieved bytes/s of the fused launch against the 8 TB/s HBM roofline;
  (b) attention at 16 heads, 4096 queries, head_dim 72: heads padded to 128 on the MFMA flash kernel against the
      one-workgroup-per-query-row fallback, self-attention (4096 keys) and cross-attention (300 keys), read in place from the
      fused projections as the model does;
  (c) one block and the 28-block forward at B = 2: text K / V cached (set_encoder_states once) against recomputed on every step,
      and one block with padded against unpadded heads.

usage: dit_bench.py [--rounds N] [--out FILE] [--sections abc] [--layers 28]"""
import argparse, ctypes as C, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from pygpukit_amd import _hip
from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import bfloat16, float32
from pygpukit_amd.core.factory import from_numpy

LINES = []


def say(s=""):
    print(s, flush=True); LINES.append(s)


def bf16(a):
    return from_numpy(np.ascontiguousarray(a, dtype=np.float32)).astype(bfloat16)


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
    """-> ({name: median us}, A' / A of the first variant, its min and max window)."""
    names = list(variants)
    for k in names: variants[k]()
    _hip.call("pgk_device_sync")
    t, again = {k: [] for k in names}, []
    for _ in range(rounds):
        for k in names: t[k].append(timer.window_us(variants[k], n))
        again.append(timer.window_us(variants[names[0]], n))
    med = {k: statistics.median(v) for k, v in t.items()}
    return med, statistics.median(again) / med[names[0]], min(t[names[0]] + again), max(t[names[0]] + again)


def section_a(timer, rounds):
    from pygpukit_amd.diffusion.ops import Modulation, gated_residual, gated_residual_adaln
    from pygpukit_amd.ops.elementwise import add, mul
    from pygpukit_amd.ops.nn.norm import layernorm

    B, N, D, eps = 2, 4096, 1152, 1e-6
    rng = np.random.default_rng(0)
    x, res = bf16(rng.standard_normal((B, N, D))), bf16(rng.standard_normal((B, N, D)))
    s, y, tmp = (GPUArray((B, N, D), bfloat16) for _ in range(3))
    table = (0.5 * rng.standard_normal((6, D))).astype(np.float32)
    cond = (0.5 * rng.standard_normal((B, 6, D))).astype(np.float32)
    dtab, dcond = from_numpy(table), from_numpy(cond)

    def m(k): return Modulation(dtab, dcond, table_offset=k * D, vector_offset=k * D, stride=6 * D)

    def bcast(k, one=0.0): return bf16(np.broadcast_to((one + table[k] + cond[:, k])[:, None, :], (B, N, D)))
    gate_b, scale_b, shift_b = bcast(2), bcast(1, 1.0), bcast(0)
    ones, zeros = bf16(np.ones(D)), bf16(np.zeros(D))
    s2, tmp2 = s._view(0, (B * N, D)), tmp._view(0, (B * N, D))

    def comp(gated, normed):
        def run():
            if gated:
                mul(x, gate_b, out=tmp); add(res, tmp, out=s)
            else:
                add(res, x, out=s)
            if normed:
                layernorm(s2, ones, zeros, eps, out=tmp2); mul(tmp, scale_b, out=tmp); add(tmp, shift_b, out=y)
        return run

    nbytes = B * N * D * 2
    say(f"(a) fused row kernel against the composition of existing ops, [{B}, {N}, {D}] bfloat16 ({nbytes / 1e6:.1f} MB per tensor)")
    for name, fused, composed, launches, passes in (
            ("gated self-attention residual (sum only)", lambda: gated_residual(res, m(2), x, out=s), comp(True, False), 2, 3),
            ("cross-attention residual + modulated norm", lambda: gated_residual_adaln(x, res, None, m(1), m(0), eps, sum_out=s, out=y), comp(False, True), 4, 4),
            ("gated FFN residual + next modulated norm", lambda: gated_residual_adaln(x, res, m(2), m(1), m(0), eps, sum_out=s, out=y), comp(True, True), 5, 4)):
        med, floor, lo, hi = measure(timer, {"fused": fused, "composed": composed}, rounds, 20)
        say(f"    {name}: fused {med['fused']:.1f} us (1 launch, {passes} tensor passes, {passes * nbytes / med['fused'] / 1e6:.2f} TB/s = "
            f"{passes * nbytes / med['fused'] / 1e6 / 8 * 100:.0f} % of 8 TB/s), composed {med['composed']:.1f} us ({launches} launches), "
            f"composed / fused {med['composed'] / med['fused']:.2f}x; fused A'/A {floor:.3f}, windows {lo:.1f}..{hi:.1f} us")


def section_b(timer, rounds):
    from pygpukit_amd.ops.nn.attention import sdpa_noncausal_strided

    H, S, M, hd = 16, 4096, 300, 72
    scale = 1.0 / np.sqrt(hd)
    rng = np.random.default_rng(1)
    say(f"(b) attention, {H} heads, {S} queries, head_dim {hd}, bfloat16, read in place from the fused projections")
    runs = {}
    for label, width in (("flash on heads padded to 128", 128), ("fallback at head_dim 72", hd)):
        dp = H * width

        def packed(rows, parts):
            a = np.zeros((rows, parts, H, width), np.float32)
            a[..., :hd] = rng.standard_normal((rows, parts, H, hd))
            return bf16(a.reshape(rows, parts * dp))
        qkv, q2, kv2 = packed(S, 3), packed(S, 1), packed(M, 2)
        out = GPUArray((S, dp), bfloat16)

        def self_attn(qkv=qkv, out=out, dp=dp, width=width):
            sdpa_noncausal_strided(qkv, qkv._view(dp, (qkv.size - dp,)), qkv._view(2 * dp, (qkv.size - 2 * dp,)), out, H, H, S, S, width,
                                   (width, 3 * dp), (width, 3 * dp), (width, dp), scale)

        def cross_attn(q2=q2, kv2=kv2, out=out, dp=dp, width=width):
            sdpa_noncausal_strided(q2, kv2, kv2._view(dp, (kv2.size - dp,)), out, H, H, S, M, width, (width, dp), (width, 2 * dp),
                                   (width, dp), scale)
        runs[label] = (self_attn, cross_attn)
    for i, kind in enumerate(("self-attention, 4096 keys", "cross-attention, 300 keys")):
        med, floor, lo, hi = measure(timer, {k: v[i] for k, v in runs.items()}, rounds, 3)
        a, b = list(med)
        say(f"    {kind}: {a} {med[a]:.1f} us, {b} {med[b]:.1f} us, fallback / padded flash {med[b] / med[a]:.2f}x; "
            f"padded flash A'/A {floor:.3f}, windows {lo:.1f}..{hi:.1f} us")


def pixart_weights(layers, rng):
    """PixArt-Sigma tensor shapes; one set of host arrays shared by every block (each block still gets its own device copy)."""
    D, T, F = 1152, 4096, 4608

    def lin(n_out, n_in): return (rng.standard_normal((n_out, n_in)) / np.sqrt(n_in)).astype(np.float32), (0.1 * rng.standard_normal(n_out)).astype(np.float32)
    w = {}

    def put(name, pair): w[name + ".weight"], w[name + ".bias"] = pair
    put("pos_embed.proj", lin(D, 16)); w["pos_embed.proj.weight"] = w["pos_embed.proj.weight"].reshape(D, 4, 2, 2)
    put("adaln_single.emb.timestep_embedder.linear_1", lin(D, 256)); put("adaln_single.emb.timestep_embedder.linear_2", lin(D, D))
    put("adaln_single.linear", lin(6 * D, D)); put("caption_projection.linear_1", lin(D, T)); put("caption_projection.linear_2", lin(D, D))
    attn, ff1, ff2 = lin(D, D), lin(F, D), lin(D, F)
    table = (0.3 * rng.standard_normal((6, D))).astype(np.float32)
    for i in range(layers):
        b = f"transformer_blocks.{i}."
        w[b + "scale_shift_table"] = table
        for a in ("attn1", "attn2"):
            for p in ("to_q", "to_k", "to_v", "to_out.0"): put(b + f"{a}.{p}", attn)
        put(b + "ff.net.0.proj", ff1); put(b + "ff.net.2", ff2)
    w["scale_shift_table"] = (0.3 * rng.standard_normal((2, D))).astype(np.float32)
    put("proj_out", lin(32, D))
    return w


def section_c(timer, rounds, layers):
    import dataclasses
    from pygpukit_amd.diffusion import PIXART_SIGMA_SPEC, PixArtTransformer, dit_plan

    rng = np.random.default_rng(2)
    B, M = 2, 300
    latent = bf16(rng.standard_normal((B, 4, 128, 128)))
    text = bf16(rng.standard_normal((B, M, 4096)))
    say(f"(c) PixArt-Sigma forward, B = {B}, 4096 tokens, {M} text tokens, bfloat16")
    w1 = pixart_weights(1, rng)
    spec1 = dataclasses.replace(PIXART_SIGMA_SPEC, num_layers=1)
    variants = {}
    for pad in (True, False):
        model = PixArtTransformer(spec1, w1, dtype="bfloat16", pad_heads=pad)
        model.set_encoder_states(text)
        variants[f"pad_heads={pad} ({model.plan['attention']})"] = (lambda model=model: model.forward(latent, 500.0))
    med, floor, lo, hi = measure(timer, variants, rounds, 2)
    a, b = list(med)
    say(f"    one block (with patch embedding, conditioning and the final layer), cached text K / V: {a} {med[a] / 1000:.2f} ms, "
        f"{b} {med[b] / 1000:.2f} ms, unpadded / padded {med[b] / med[a]:.2f}x; A'/A {floor:.3f}, windows {lo / 1000:.2f}..{hi / 1000:.2f} ms")
    del variants, model
    plan = dit_plan(PIXART_SIGMA_SPEC, "bfloat16", "auto")
    model = PixArtTransformer(dataclasses.replace(PIXART_SIGMA_SPEC, num_layers=layers), pixart_weights(layers, rng), dtype="bfloat16")
    model.set_encoder_states(text)
    med, floor, lo, hi = measure(timer, {"cached": lambda: model.forward(latent, 500.0), "recomputed": lambda: model.forward(latent, 500.0, text)},
                                 rounds, 1)
    say(f"    {layers} blocks, pad_heads='auto' -> {plan}: text K / V cached {med['cached'] / 1000:.2f} ms per step, recomputed "
        f"{med['recomputed'] / 1000:.2f} ms, recomputed / cached {med['recomputed'] / med['cached']:.3f}x; cached A'/A {floor:.3f}, "
        f"windows {lo / 1000:.2f}..{hi / 1000:.2f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "r15_dit_bench.log"))
    ap.add_argument("--sections", default="abc")
    ap.add_argument("--layers", type=int, default=28)
    args = ap.parse_args()
    props = _hip.DeviceProps(); _hip.call("pgk_device_props", 0, C.byref(props))
    say(f"dit_bench: {props.name.decode()} ({props.arch.decode()}), {args.rounds} rounds, {time.strftime('%Y-%m-%d')}")
    timer = Timer()
    if "a" in args.sections: section_a(timer, args.rounds)
    if "b" in args.sections: section_b(timer, args.rounds)
    if "c" in args.sections: section_c(timer, args.rounds, args.layers)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f: f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
