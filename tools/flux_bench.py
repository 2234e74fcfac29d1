"""Time the FLUX path at FLUX.1's shape (hidden 3072, 24 heads of 128, 512 text + 4096 image tokens = 1024 px, 19 double + 38
single blocks), bfloat16, B = 1, in one process with alternating windows: per round every variant of a section once, then the
first variant again (A'), N calls each between device events after a warm-up of all of them.  Prints the median us per call and
the spread of the first variant against itself (A' / A: the margin inside which two numbers are "the same").  Not a pass / fail gate.

  (a) flux_qk_norm_rope on the joint [4608, 9216] q|k|v buffer (split 512), with the bytes it must move (Q and K read and
      written, the two fp32 tables read) per second, beside copy_to of a buffer of the Q + K bytes in the same run;
  (b) flux_gelu_pack of [4608, 12288] into columns 3072.. of [4608, 15360] against gelu followed by copy_to of the same bytes
      into a CONTIGUOUS buffer (the library has no strided copy, so the composition is timed at its lower bound);
  (c) one double block and one single block, as the difference of a 3-block and a 1-block forward divided by two;
  (d) a full 19 + 38 step, and the parts timed on their own at the step's shapes and counts: the modulation projection, the
      57 attentions, the row kernels (57 norm-rope, 38 gelu_pack, 114 gated_residual_adaln); the GEMMs are the remainder.
The blocks of (c) and (d) ALIAS one double block's and one single block's synthetic weights (the host does not have to draw 12 G
numbers) and the packed modulation matrix is zero-filled on the device with a random bias; GEMM and row-kernel time does not
depend on the values.

usage: flux_bench.py [--rounds N] [--out FILE] [--sections abcd]"""
import argparse, ctypes as C, dataclasses, os, statistics, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from pygpukit_amd import _hip
from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import bfloat16, float32
from pygpukit_amd.core.factory import from_numpy

LINES = []
D, H, HD, T, I = 3072, 24, 128, 512, 4096
S = T + I


def say(s=""):
    print(s, flush=True); LINES.append(s)


def draw(rng, shape, std=1.0):
    return (std * rng.standard_normal(shape, dtype=np.float32))


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


def norm_rope_call(rng):
    from pygpukit_amd.diffusion.ops import flux_qk_norm_rope
    qkv = bf16(draw(rng, (S, 3 * D)))
    w = [from_numpy(1 + 0.1 * draw(rng, (HD,))) for _ in range(4)]
    cos, sin = from_numpy(draw(rng, (S, HD))), from_numpy(draw(rng, (S, HD)))
    k = qkv._view(D, (qkv.size - D,))
    return qkv, lambda: flux_qk_norm_rope(qkv, k, cos, sin, w[0], w[1], batch=1, seq=S, heads=H, head_dim=HD, row_stride=3 * D, split=T,
                                          wq_b=w[2], wk_b=w[3])


def section_a(timer, rounds):
    from pygpukit_amd.diffusion.ops import flux_qk_norm_rope_plan
    from pygpukit_amd.ops.elementwise import copy_to
    rng = np.random.default_rng(0)
    qkv, run = norm_rope_call(rng)
    qk_bytes = S * 2 * D * 2
    src, dst = bf16(draw(rng, (S, 2 * D))), GPUArray((S, 2 * D), bfloat16)
    moved = 2 * qk_bytes + 2 * S * HD * 4
    med, floor, lo, hi = measure(timer, {"norm_rope": run, "copy_to": lambda: copy_to(src, dst)}, rounds, 20)
    say(f"(a) flux_qk_norm_rope ({flux_qk_norm_rope_plan(HD, 'bfloat16')}) on the joint [{S}, {3 * D}] bfloat16 buffer, split {T}: "
        f"{med['norm_rope']:.1f} us, {moved / 1e6:.1f} MB to move = {moved / med['norm_rope'] / 1e6:.2f} TB/s; copy_to of the Q + K bytes "
        f"({qk_bytes / 1e6:.1f} MB read + as many written) {med['copy_to']:.1f} us = {2 * qk_bytes / med['copy_to'] / 1e6:.2f} TB/s; "
        f"norm_rope / copy_to {med['norm_rope'] / med['copy_to']:.2f}x; A'/A {floor:.3f}, windows {lo:.1f}..{hi:.1f} us")


def section_b(timer, rounds):
    from pygpukit_amd.diffusion.ops import flux_gelu_pack
    from pygpukit_amd.ops.elementwise import copy_to
    from pygpukit_amd.ops.nn.activation import gelu
    rng = np.random.default_rng(1)
    M = 4 * D
    x, cat = bf16(draw(rng, (S, M))), GPUArray((S, D + M), bfloat16)
    tmp, flat = GPUArray((S, M), bfloat16), GPUArray((S, M), bfloat16)

    def composed():
        gelu(x, out=tmp); copy_to(tmp, flat)
    nbytes = S * M * 2
    med, floor, lo, hi = measure(timer, {"gelu_pack": lambda: flux_gelu_pack(x, cat, column=D), "gelu + copy_to": composed}, rounds, 10)
    say(f"(b) flux_gelu_pack [{S}, {M}] -> columns {D}.. of [{S}, {D + M}] bfloat16: {med['gelu_pack']:.1f} us "
        f"({2 * nbytes / med['gelu_pack'] / 1e6:.2f} TB/s of {2 * nbytes / 1e6:.0f} MB); gelu + copy_to into a contiguous buffer "
        f"{med['gelu + copy_to']:.1f} us (2 launches, {4 * nbytes / 1e6:.0f} MB); composed / packed {med['gelu + copy_to'] / med['gelu_pack']:.2f}x; "
        f"A'/A {floor:.3f}, windows {lo:.1f}..{hi:.1f} us")


def base_weights(rng, cfg):
    """One double and one single block of FLUX.1 shapes and everything outside the blocks."""
    w = {}

    def lin(name, n_out, n_in):
        w[name + ".weight"], w[name + ".bias"] = draw(rng, (n_out, n_in), 1 / np.sqrt(n_in)), draw(rng, (n_out,), 0.1)
    lin("x_embedder", D, cfg.in_channels); lin("context_embedder", D, cfg.joint_attention_dim); lin("proj_out", cfg.in_channels, D)
    for g, n_in in (("timestep_embedder", 256), ("text_embedder", cfg.pooled_projection_dim)):
        lin(f"time_text_embed.{g}.linear_1", D, n_in); lin(f"time_text_embed.{g}.linear_2", D, D)
    p = "transformer_blocks.0."
    lin(p + "norm1.linear", 6 * D, D); lin(p + "norm1_context.linear", 6 * D, D)
    for n in ("to_q", "to_k", "to_v", "add_q_proj", "add_k_proj", "add_v_proj", "to_out.0", "to_add_out"): lin(p + "attn." + n, D, D)
    for ff in ("ff", "ff_context"): lin(p + ff + ".net.0.proj", 4 * D, D); lin(p + ff + ".net.2", D, 4 * D)
    s = "single_transformer_blocks.0."
    lin(s + "norm.linear", 3 * D, D)
    for n in ("to_q", "to_k", "to_v"): lin(s + "attn." + n, D, D)
    lin(s + "proj_mlp", 4 * D, D); lin(s + "proj_out", D, 5 * D)
    lin("norm_out.linear", 2 * D, D)
    for n in (p + "attn.norm_q", p + "attn.norm_k", p + "attn.norm_added_q", p + "attn.norm_added_k", s + "attn.norm_q", s + "attn.norm_k"):
        w[n + ".weight"] = 1 + 0.1 * draw(rng, (HD,))
    return w


def aliased(base, L, Ls, rng):
    """A view of `base` (a 1 + 1 block model) with L double and Ls single blocks that alias its two blocks' weights."""
    import copy
    from pygpukit_amd.diffusion.models.flux.model import flux_plan, modulation_layout
    m = copy.copy(base)
    m.config = dataclasses.replace(base.config, num_layers=L, num_single_layers=Ls)
    m.double, m.single = [base.double[0]] * L, [base.single[0]] * Ls
    m.layout = modulation_layout(m.config)
    m.plan = flux_plan(m.config, "bfloat16")
    m.mod_w = GPUArray((m.layout["rows"], D), bfloat16); m.mod_w.fill_zeros()
    m.mod_b = bf16(draw(rng, (m.layout["rows"],), 0.3))
    m._rope = base._rope
    return m


def section_cd(timer, rounds, sections):
    from pygpukit_amd.diffusion import FluxConfig, FluxTransformer
    from pygpukit_amd.diffusion.models.flux.embeddings import prepare_image_ids, prepare_text_ids
    from pygpukit_amd.diffusion.ops import Modulation, flux_gelu_pack, gated_residual_adaln
    from pygpukit_amd.ops.matmul import matmul_nt
    from pygpukit_amd.ops.nn.activation import silu
    from pygpukit_amd.ops.nn.attention import sdpa_noncausal_strided
    rng = np.random.default_rng(2)
    cfg = FluxConfig(num_layers=1, num_single_layers=1)
    base = FluxTransformer(cfg, base_weights(rng, cfg), dtype="bfloat16")
    base.set_encoder_states(bf16(draw(rng, (1, T, cfg.joint_attention_dim))), from_numpy(draw(rng, (1, cfg.pooled_projection_dim))))
    hidden = bf16(draw(rng, (1, I, cfg.in_channels)))
    ids = dict(img_ids=prepare_image_ids(1, 64, 64), txt_ids=prepare_text_ids(1, T))
    t = np.array([500.0], np.float32)

    def step(m): return lambda: m.forward(hidden, timestep=t, **ids)
    if "c" in sections:
        models = {f"{L}+{Ls}": aliased(base, L, Ls, rng) for L, Ls in ((1, 0), (3, 0), (0, 1), (0, 3))}
        med, floor, lo, hi = measure(timer, {k: step(m) for k, m in models.items()}, rounds, 2)
        say(f"(c) forwards of aliased blocks, [{T} text + {I} image tokens, hidden {D}], bfloat16, B = 1: " +
            ", ".join(f"{k} blocks {v / 1000:.2f} ms" for k, v in med.items()) +
            f"; one double block {(med['3+0'] - med['1+0']) / 2000:.2f} ms (16 launches), one single block "
            f"{(med['0+3'] - med['0+1']) / 2000:.2f} ms (7 launches); 1+0 A'/A {floor:.3f}, windows {lo / 1000:.2f}..{hi / 1000:.2f} ms")
        del models
    if "d" in sections:
        full = aliased(base, 19, 38, rng)
        med, floor, lo, hi = measure(timer, {"step": step(full)}, max(3, rounds // 2), 1)
        say(f"(d) full step, 19 double + 38 single blocks (aliased weights, zero modulation matrix), plan {full.plan}: "
            f"{med['step'] / 1000:.1f} ms; A'/A {floor:.3f}, windows {lo / 1000:.1f}..{hi / 1000:.1f} ms")
        temb = from_numpy(draw(rng, (1, D)))

        def modulation():
            matmul_nt(silu(temb).astype(bfloat16), full.mod_w, full.mod_b)
        qkv, norm_rope = norm_rope_call(rng)
        out = GPUArray((S, D), bfloat16)

        def attention():
            sdpa_noncausal_strided(qkv, qkv._view(D, (qkv.size - D,)), qkv._view(2 * D, (qkv.size - 2 * D,)), out, H, H, S, S, HD,
                                   (HD, 3 * D), (HD, 3 * D), (HD, D), 1.0 / np.sqrt(HD))
        mlp, cat = bf16(draw(rng, (S, 4 * D))), GPUArray((S, 5 * D), bfloat16)
        x, res, y = bf16(draw(rng, (1, S, D))), bf16(draw(rng, (1, S, D))), GPUArray((1, S, D), bfloat16)
        proj = bf16(draw(rng, (3 * D,)))

        def mod(k): return Modulation(vector=proj, vector_offset=k * D, stride=0)

        def adaln():
            gated_residual_adaln(x, res, mod(2), mod(1), mod(0), 1e-6, sum_out=res, out=y)
        parts, _, _, _ = measure(timer, {"modulation": modulation, "attention": attention, "norm_rope": norm_rope,
                                        "gelu_pack": lambda: flux_gelu_pack(mlp, cat, column=D), "adaln": adaln}, rounds, 5)
        # a double block runs its four row kernels on 512 + 4096 rows: two launches over the joint row count move the same bytes
        rows = 57 * parts["norm_rope"] + 38 * parts["gelu_pack"] + (2 * 19 + 38) * parts["adaln"]
        attn = 57 * parts["attention"]
        rest = med["step"] - parts["modulation"] - attn - rows
        say(f"    parts on their own at the step's shapes: modulation projection (silu + cast + [{full.layout['rows']}, {D}] GEMM) "
            f"{parts['modulation']:.0f} us; attention {parts['attention']:.0f} us x 57 = {attn / 1000:.1f} ms; row kernels "
            f"{rows / 1000:.1f} ms (norm_rope {parts['norm_rope']:.0f} us x 57, gelu_pack {parts['gelu_pack']:.0f} us x 38, "
            f"gated_residual_adaln on {S} rows {parts['adaln']:.0f} us x 76); GEMMs, GELUs of the FFNs and everything else by "
            f"difference {rest / 1000:.1f} ms = {rest / med['step'] * 100:.0f} % of the step")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "r17_flux_bench.log"))
    ap.add_argument("--sections", default="abcd")
    args = ap.parse_args()
    props = _hip.DeviceProps(); _hip.call("pgk_device_props", 0, C.byref(props))
    say(f"flux_bench on {props.name.decode()} ({props.cu_count} CUs), rounds {args.rounds}, bfloat16")
    timer = Timer()
    if "a" in args.sections: section_a(timer, args.rounds)
    if "b" in args.sections: section_b(timer, args.rounds)
    if "c" in args.sections or "d" in args.sections: section_cd(timer, args.rounds, args.sections)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
