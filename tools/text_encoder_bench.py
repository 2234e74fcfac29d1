"""Time the text-encoder path in one process with alternating windows: per round every variant of a section once, then the first
variant again (A'), N calls each between device events after a warm-up of all of them.  Prints the median us per call and the
spread of the first variant against itself (A' / A: the margin inside which two numbers are "the same").  Not a pass / fail gate.

  (a) sdpa_relbias at T5-XXL's attention shape (64 heads of 64, 512 tokens) and at 16 heads of 128, bfloat16, radius 128, against
      sdpa_noncausal on the same tensors (the price of the bias) and against the composition that materialises the dense bias on
      existing ops: batched_matmul Q K^T (one GEMM per head), add of the [H, S, S] bias, softmax, batched_matmul with V;
  (b) one T5-XXL-shaped layer (hidden 4096, 64 heads of 64, d_ff 10240) at 512 tokens, bfloat16, as the difference of a 3-layer and
      a 1-layer forward divided by two, and the 24-layer forward; every layer ALIASES one layer's synthetic weights (GEMM and row
      kernel time does not depend on the values);
  (c) the CLIP-L forward (768 wide, 12 layers, 12 heads of 64) at 77 tokens, bfloat16.

usage: text_encoder_bench.py [--rounds N] [--out FILE] [--sections abc]"""
import argparse, copy, ctypes as C, os, statistics, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from pygpukit_amd import _hip
from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import bfloat16
from pygpukit_amd.core.factory import from_numpy

LINES = []


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


def section_a(timer, rounds):
    from pygpukit_amd.ops.elementwise import add
    from pygpukit_amd.ops.matmul import batched_matmul
    from pygpukit_amd.ops.nn import relbias_plan, relpos_bias_table, relpos_compute_bias, sdpa_noncausal, sdpa_relbias
    from pygpukit_amd.ops.reduction import softmax
    rng = np.random.default_rng(0)
    for H, S, D in ((64, 512, 64), (16, 512, 128)):
        q, k, v = (bf16(draw(rng, (H, S, D), D ** -0.25 if i < 2 else 1.0)) for i in range(3))
        kt = bf16(np.ascontiguousarray(draw(rng, (H, D, S), D ** -0.25)))
        table = relpos_bias_table(draw(rng, (32, H), 1.5))
        dense = relpos_compute_bias(table, S, S).astype(bfloat16)
        out = GPUArray((H, S, D), bfloat16)

        def composed():
            batched_matmul(softmax(add(batched_matmul(q, kt), dense)), v)
        med, floor, lo, hi = measure(timer, {"relbias": lambda: sdpa_relbias(q, k, v, table, 1.0, out=out),
                                             "noncausal": lambda: sdpa_noncausal(q, k, v, 1.0, out=out), "composed": composed}, rounds, 10)
        flops = 4.0 * H * S * S * D
        k_reads, bias_reads = 2 * (D // 16), 32       # LDS read instructions per lane and KV tile: ds_read_b128 of K, ds_read_b32 of the table
        say(f"(a) sdpa_relbias ({relbias_plan(D, 128, 'bfloat16')}) H {H} S {S} D {D} bfloat16, radius 128, scale 1.0: {med['relbias']:.1f} us "
            f"({flops / med['relbias'] / 1e6:.1f} TFLOP/s); sdpa_noncausal {med['noncausal']:.1f} us: the bias costs "
            f"{med['relbias'] / med['noncausal']:.3f}x ({med['relbias'] - med['noncausal']:+.1f} us; per near tile a lane issues {bias_reads} table reads of 4 "
            f"bytes beside {k_reads} K reads of 16); composition with the dense [{H}, {S}, {S}] bias ({2 * H} GEMM launches + add + softmax, "
            f"{H * S * S * 2 / 1e6:.0f} MB of scores three times over) {med['composed']:.1f} us = {med['composed'] / med['relbias']:.2f}x the fused "
            f"kernel; A'/A {floor:.3f}, windows {lo:.1f}..{hi:.1f} us")


def t5_xxl(rng, layers):
    """A T5-XXL-shaped encoder of `layers` layers that all alias one layer's weights."""
    from pygpukit_amd.diffusion import T5Encoder
    D, H, DK, DFF = 4096, 64, 64, 10240
    w = {"shared.weight": draw(rng, (512, D)), "encoder.final_layer_norm.weight": 1 + 0.1 * draw(rng, (D,))}
    p = "encoder.block.0.layer"
    for n in "qk": w[f"{p}.0.SelfAttention.{n}.weight"] = draw(rng, (H * DK, D), 1 / np.sqrt(D * 8))
    w[f"{p}.0.SelfAttention.v.weight"] = draw(rng, (H * DK, D), 1 / np.sqrt(D))
    w[f"{p}.0.SelfAttention.o.weight"] = draw(rng, (D, H * DK), 1 / np.sqrt(H * DK))
    w[f"{p}.0.SelfAttention.relative_attention_bias.weight"] = draw(rng, (32, H), 1.5)
    for n in ("wi_0", "wi_1"): w[f"{p}.1.DenseReluDense.{n}.weight"] = draw(rng, (DFF, D), 1 / np.sqrt(D))
    w[f"{p}.1.DenseReluDense.wo.weight"] = draw(rng, (D, DFF), 1 / np.sqrt(DFF))
    for i in (0, 1): w[f"{p}.{i}.layer_norm.weight"] = 1 + 0.1 * draw(rng, (D,))
    one = T5Encoder(hidden_size=D, num_layers=1, num_heads=H, d_ff=DFF, weights=w, dtype="bfloat16")

    def with_layers(n):
        m = copy.copy(one)
        m.layers, m.num_layers = [one.layers[0]] * n, n
        return m
    return {n: with_layers(n) for n in layers}


def section_b(timer, rounds):
    rng = np.random.default_rng(1)
    S = 512
    models = t5_xxl(rng, (1, 3, 24))
    ids = rng.integers(0, 512, (1, S))
    med, floor, lo, hi = measure(timer, {f"{n} layers": (lambda m=m: m.forward(ids)) for n, m in models.items()}, rounds, 2)
    layer = (med["3 layers"] - med["1 layers"]) / 2
    plan = models[24].plan(S)
    gemm_flops = 2.0 * S * 4096 * (3 * 4096 + 4096 + 2 * 10240 + 10240)
    say(f"(b) T5-XXL-shaped encoder, {S} tokens, bfloat16, B = 1 ({plan['launches_per_layer']} op launches per layer, attention {plan['attention']}, "
        f"bias table {plan['table_bytes'] / 1024:.0f} KiB once against a dense bias of {plan['dense_bias_bytes'] / 1e6:.0f} MB per layer in the "
        f"reference): one layer {layer:.0f} us ({gemm_flops / layer / 1e6:.0f} TFLOP/s of GEMM work); 1 layer + embedding + final norm "
        f"{med['1 layers']:.0f} us; 24 layers {med['24 layers'] / 1000:.2f} ms ({med['24 layers'] / 24:.0f} us per layer); A'/A {floor:.3f}, "
        f"windows {lo:.0f}..{hi:.0f} us")


def section_c(timer, rounds):
    from pygpukit_amd.diffusion import CLIPTextEncoderL
    rng = np.random.default_rng(2)
    D, L, FF = 768, 12, 3072
    w = {"text_model.embeddings.token_embedding.weight": draw(rng, (49408, D)), "text_model.embeddings.position_embedding.weight": draw(rng, (77, D), 0.5)}

    def lin(name, n_out, n_in):
        w[name + ".weight"], w[name + ".bias"] = draw(rng, (n_out, n_in), 1 / np.sqrt(n_in)), draw(rng, (n_out,), 0.1)

    def norm(name):
        w[name + ".weight"], w[name + ".bias"] = 1 + 0.1 * draw(rng, (D,)), 0.1 * draw(rng, (D,))
    for i in range(L):
        p = f"text_model.encoder.layers.{i}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"): lin(p + "self_attn." + n, D, D)
        lin(p + "mlp.fc1", FF, D); lin(p + "mlp.fc2", D, FF); norm(p + "layer_norm1"); norm(p + "layer_norm2")
    norm("text_model.final_layer_norm")
    enc = CLIPTextEncoderL(weights=w, dtype="bfloat16")
    ids, _ = enc.tokenize("a photo of a cat sitting on a mat")
    med, floor, lo, hi = measure(timer, {"clip_l": lambda: enc.forward(ids)}, rounds, 5)
    say(f"(c) CLIP-L text encoder, 77 tokens, bfloat16, B = 1 (12 layers, 9 op launches + 4 casts to and from the float32 residual stream each): {med['clip_l']:.0f} us per forward "
        f"({med['clip_l'] / 12:.0f} us per layer); A'/A {floor:.3f}, windows {lo:.0f}..{hi:.0f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sections", default="abc")
    a = ap.parse_args()
    timer = Timer()
    for s, fn in (("a", section_a), ("b", section_b), ("c", section_c)):
        if s in a.sections:
            fn(timer, a.rounds)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
