"""Time the Whisper decoder's one-token step against what the project could run before it, in one process with alternating
windows: per round every variant once, then the first again (A .. A'), N calls each between device events after a warm-up of all
of them.  Prints medians in us per generated token, the ratios, and each variant against itself (A' / A and min..max of its
windows: the margin inside which two numbers are "the same").  bf16, d_model 1280, 20 heads, FFN 5120, vocabulary 51866, 1500
encoder rows; 32 layers (Whisper-large-v3) and 2 layers (the distilled shape); contexts 32 and 224.

  (a) uncached: the teacher-forced forward over the whole prefix (use_cache=False generates one token per such call)
  (b) cached step, fused=False: layernorm, matmul_nt, gelu, add, cache-write ops (19 launches per layer + 6)
  (c) cached step, fused=True, eager (10 launches per layer + 3)
  (d) the same step replayed as one graph
Every cached variant includes its 12-byte state upload.  (b) and (c) are first checked against each other (rel_err of the logits).

Also: ln_linear alone against the composition of existing ops on [1,1280] -> 5120 with LN + GELU and on [1,5120] -> 1280 with a
residual, and at eight rows; ln_linear alone on [1,1280] -> 51866 in TB/s of weight bytes; set_encoder_states once.
One layer's random weights are reused for every layer (each layer uploads its own copy, so the bytes streamed are the model's).
usage: whisper_decoder_bench.py [--rounds N] [--layers 32,2]"""
import ctypes as C, os, statistics, sys, numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from pygpukit_amd import _hip, ops
from pygpukit_amd.asr.whisper import WhisperConfig, WhisperWeights, create_decoder
from pygpukit_amd.core import GPUArray, bfloat16, from_numpy

D, HEADS, FFN, VOCAB, S_ENC, MAX_POS = 1280, 20, 5120, 51866, 1500, 448


def dev(a, dt=bfloat16):
    return from_numpy(np.ascontiguousarray(a, np.float32)).astype(dt)


def host(a):
    h = a.to_numpy()
    return (h.astype(np.uint32) << 16).view(np.float32) if h.dtype == np.uint16 else h.astype(np.float32)


def rel(a, b):
    a, b = host(a).astype(np.float64).ravel(), host(b).astype(np.float64).ravel()
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def window_us(run, e0, e1, n):
    _hip.call("pgk_event_record", e0, None)
    for _ in range(n): run()
    _hip.call("pgk_event_record", e1, None); _hip.call("pgk_event_sync", e1)
    ms = C.c_float(); _hip.call("pgk_event_elapsed_ms", e0, e1, C.byref(ms))
    return ms.value * 1000 / n


def race(variants, e0, e1, rounds):
    """variants: [(name, run, calls per window)] -> {name: (median us, A'/A, min, max)}; every variant is timed twice per round,
    once on the way through the list and once on the way back, so drift hits all of them alike."""
    for _, run, _ in variants:
        for _ in range(3): run()
    _hip.call("pgk_device_sync")
    first, second = {n: [] for n, _, _ in variants}, {n: [] for n, _, _ in variants}
    for _ in range(rounds):
        for name, run, n in variants: first[name].append(window_us(run, e0, e1, n))
        for name, run, n in reversed(variants): second[name].append(window_us(run, e0, e1, n))
    _hip.call("pgk_device_sync")
    med = statistics.median
    return {n: (med(first[n] + second[n]), med(second[n]) / med(first[n]), min(first[n] + second[n]), max(first[n] + second[n])) for n, _, _ in variants}


def show(title, res):
    print(title, flush=True)
    for name, (m, self_ratio, lo, hi) in res.items():
        print(f"    {name:<28} {m:10.1f} us   (against itself A'/A {self_ratio:6.4f}, windows {lo:.1f} .. {hi:.1f} us)", flush=True)


def make_weights(cfg, rng):
    mat = lambda r, c: (rng.standard_normal((r, c), dtype=np.float32) / np.float32(np.sqrt(c)))
    vec = lambda n, m=0.0: (m + 0.1 * rng.standard_normal(n)).astype(np.float32)
    layer = {}
    for a in ("self_attn", "cross_attn"):
        for p in ("q", "k", "v", "out"):
            layer[f"{a}_{p}_weight"] = mat(D, D)
            layer[f"{a}_{p}_bias"] = None if p == "k" else vec(D)
        layer[f"{a}_layer_norm_weight"], layer[f"{a}_layer_norm_bias"] = vec(D, 1.0), vec(D)
    layer.update(fc1_weight=mat(FFN, D), fc1_bias=vec(FFN), fc2_weight=mat(D, FFN), fc2_bias=vec(D),
                 final_layer_norm_weight=vec(D, 1.0), final_layer_norm_bias=vec(D))
    w = WhisperWeights(cfg)
    w.decoder_embed_tokens = rng.standard_normal((VOCAB, D), dtype=np.float32)
    w.decoder_embed_positions = rng.standard_normal((MAX_POS, D), dtype=np.float32)
    w.decoder_layer_norm_weight, w.decoder_layer_norm_bias = vec(D, 1.0), vec(D)
    w.proj_out_weight = mat(VOCAB, D)
    w.decoder_layers = [layer] * cfg.decoder_layers
    return w


def model(layers, e0, e1, rounds):
    cfg = WhisperConfig(d_model=D, decoder_layers=layers, decoder_attention_heads=HEADS, decoder_ffn_dim=FFN, vocab_size=VOCAB,
                        max_source_positions=S_ENC, max_target_positions=MAX_POS)
    rng = np.random.default_rng(layers)
    w = make_weights(cfg, rng)
    fused, plain = create_decoder(cfg, w, bfloat16, fused=True), create_decoder(cfg, w, bfloat16, fused=False)
    enc = dev(rng.standard_normal((1, S_ENC, D), dtype=np.float32))
    fused.set_encoder_states(enc)                                          # warm-up: allocates the cross caches and the workspace
    t = statistics.median([window_us(lambda: fused.set_encoder_states(enc), e0, e1, 1) for _ in range(5)])
    print(f"{layers} layers: set_encoder_states ({S_ENC} rows, once per audio) {t:.0f} us", flush=True)
    plain.set_encoder_states(enc)
    fused.capture_decode()
    tokens = [int(v) for v in rng.integers(0, VOCAB, 224)]
    for pos, tok in enumerate(tokens):                      # fill the self caches of both with the same prefix
        lf, lp = fused.decode_step(tok, pos), plain.decode_step(tok, pos)
    print(f"{layers} layers: launches per step fused {fused.decode_launches()}, unfused {plain.decode_launches()}; "
          f"logits fused vs unfused at position 223: rel_err {rel(lf, lp):.2e}; graph nodes {fused._graph.num_nodes}", flush=True)
    for ctx in (32, 224):
        ids = np.array([tokens[:ctx]], dtype=np.int64)
        pos, tok = ctx - 1, tokens[ctx - 1]
        res = race([("(c) fused eager", lambda: fused.decode_step(tok, pos), 20),
                    ("(b) unfused cached", lambda: plain.decode_step(tok, pos), 20),
                    ("(d) fused graph", lambda: fused.decode_step_graph(tok, pos), 20),
                    ("(a) uncached forward", lambda: fused(ids, enc), 2)], e0, e1, rounds)
        show(f"{layers} layers, context {ctx}, bf16, us per generated token:", res)
        a, b, c, d = (res[k][0] for k in ("(a) uncached forward", "(b) unfused cached", "(c) fused eager", "(d) fused graph"))
        print(f"    c / b {c / b:.3f}   d / b {d / b:.3f}   b / a {b / a:.4f}   d / c {d / c:.3f}", flush=True)


def ops_alone(e0, e1, rounds):
    rng = np.random.default_rng(9)
    mat = lambda r, c: dev(rng.standard_normal((r, c), dtype=np.float32) / np.float32(np.sqrt(c)))
    vec = lambda n, m=0.0: dev(m + 0.1 * rng.standard_normal(n))
    x, g, be = dev(0.3 + rng.standard_normal((1, D))), vec(D, 1.0), vec(D)
    w1, b1, w2, b2 = mat(FFN, D), vec(FFN), mat(D, FFN), vec(D)
    h, r = dev(rng.standard_normal((1, FFN))), dev(rng.standard_normal((1, D)))
    o1, o1b, n1 = GPUArray((1, FFN), bfloat16), GPUArray((1, FFN), bfloat16), GPUArray((1, D), bfloat16)
    o2, o2b = GPUArray((1, D), bfloat16), GPUArray((1, D), bfloat16)

    def old1():
        ops.layernorm(x, g, be, out=n1); ops.matmul_nt(n1, w1, b1, out=o1b); return ops.gelu(o1b, out=o1b)

    def old2():
        ops.matmul_nt(h, w2, b2, out=o2b); return ops.add(o2b, r, out=o2b)

    new1 = lambda: ops.ln_linear(x, w1, b1, gamma=g, beta=be, activation="gelu", out=o1)
    new2 = lambda: ops.ln_linear(h, w2, b2, residual=r, out=o2)
    print(f"ln_linear vs composition: rel_err {rel(new1(), old1()):.2e} (LN + GELU), {rel(new2(), old2()):.2e} (residual)", flush=True)
    res = race([("ln_linear 1280->5120 LN+GELU", new1, 200), ("layernorm+matmul_nt+gelu", old1, 200)], e0, e1, rounds)
    show("[1,1280] -> 5120, LN + bias + GELU, bf16:", res)
    res = race([("ln_linear 5120->1280 +res", new2, 200), ("matmul_nt+add", old2, 200)], e0, e1, rounds)
    show("[1,5120] -> 1280, bias + residual, bf16:", res)
    # eight rows: every activation read of the fp32 image is a 2-way LDS bank conflict (32 bytes per lane at a 32-byte stride)
    x8, o8, o8b, n8 = dev(0.3 + rng.standard_normal((8, D))), GPUArray((8, FFN), bfloat16), GPUArray((8, FFN), bfloat16), GPUArray((8, D), bfloat16)
    new8 = lambda: ops.ln_linear(x8, w1, b1, gamma=g, beta=be, activation="gelu", out=o8)

    def old8():
        ops.layernorm(x8, g, be, out=n8); ops.matmul_nt(n8, w1, b1, out=o8b); return ops.gelu(o8b, out=o8b)

    print(f"ln_linear vs composition at 8 rows: rel_err {rel(new8(), old8()):.2e}", flush=True)
    res = race([("ln_linear [8,1280]->5120", new8, 200), ("layernorm+matmul_nt+gelu", old8, 200)], e0, e1, rounds)
    show("[8,1280] -> 5120, LN + bias + GELU, bf16:", res)
    wv, ov = mat(VOCAB, D), GPUArray((1, VOCAB), bfloat16)
    res = race([("ln_linear 1280->51866 LN", lambda: ops.ln_linear(x, wv, None, gamma=g, beta=be, out=ov), 50),
                ("layernorm+matmul_nt", lambda: (ops.layernorm(x, g, be, out=n1), ops.matmul_nt(n1, wv, out=ov)), 50)], e0, e1, rounds)
    show("[1,1280] -> 51866, final LN + output projection, bf16:", res)
    us = res["ln_linear 1280->51866 LN"][0]
    print(f"    ln_linear alone: {VOCAB * D * 2 / us / 1e6:.2f} TB/s of weight bytes", flush=True)


def main():
    args = sys.argv[1:]
    rounds, layers = 7, (32, 2)
    if "--rounds" in args: rounds = int(args[args.index("--rounds") + 1])
    if "--layers" in args: layers = tuple(int(v) for v in args[args.index("--layers") + 1].split(","))
    _hip.require_device()
    e0, e1 = C.c_void_p(), C.c_void_p()
    _hip.call("pgk_event_create", C.byref(e0)); _hip.call("pgk_event_create", C.byref(e1))
    ops_alone(e0, e1, rounds)
    for n in layers:
        model(n, e0, e1, rounds)
    return 0


if __name__ == "__main__":
    sys.exit(main())
