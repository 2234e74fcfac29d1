"""Time Llama-4 decode with and without the KV cache, and the cached attention op against the composition it replaces, in
one process with alternating windows.

Model: Scout-shaped blocks (hidden 5120, Hq 40 / Hkv 8 / D 128, intermediate 8192), --layers of them (default 4), a small
vocabulary (8192: the lm_head is not what is compared), seeded bf16 weights.  Per context length (default 512 and 4096),
ms per generated token, host clock around calls that end in a device synchronise:
  (a) forward on the whole sequence - what generate() does without the cache;
  (b) decode_step        - eager one-token step against the prefilled cache;
  (c) decode_step_graph  - the same step as one graph replay;
per round a, b, c, a again (a'), the medians, b / a and c / a, and the spread of (a) against itself.
Op: per round composition (A), sdpa_irope_fixed_cache, composition again (A') between device events, where the composition
is pgk_irope_scale_q + pgk_sdpa_fixed_cache on the same tensors (position = context - 1, cache of `context` rows); the
composition's spread against itself is the margin inside which the ratio means "the same".
usage: llama4_decode_bench.py [--rounds N] [--layers L] [context ...]     (default: 512 4096, and 16384 for the op alone)"""
import ctypes as C, os, statistics, sys, time, numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from pygpukit_amd import _hip
from pygpukit_amd.core import from_numpy
from pygpukit_amd.llm.models.llama4 import Llama4Attention, Llama4Block, Llama4Config, Llama4MLP, Llama4Model

HQ, HKV, D, HIDDEN, INTER, VOCAB = 40, 8, 128, 5120, 8192, 8192
PGK_BF16, PGK_I32 = 3, 5      # pgk_dtype, include/pgk_hip.h


def bf16_bits(rng, shape, scale=1.0):
    x = (rng.standard_normal(shape, dtype=np.float32) * np.float32(scale)).view(np.uint32)
    return ((x + 0x7FFF + ((x >> 16) & 1)) >> 16).astype(np.uint16)


def build_model(layers):
    rng = np.random.default_rng(0)
    cfg = Llama4Config(vocab_size=VOCAB, hidden_size=HIDDEN, intermediate_size=INTER, num_hidden_layers=layers,
                       num_attention_heads=HQ, num_key_value_heads=HKV, head_dim=D)
    lin = lambda o, i: bf16_bits(rng, (o, i), 1.0 / np.sqrt(i))
    # one set of host weights, uploaded once per layer: every layer streams its own device copy
    host = dict(q=lin(HQ * D, HIDDEN), k=lin(HKV * D, HIDDEN), v=lin(HKV * D, HIDDEN), o=lin(HIDDEN, HQ * D),
                gate=lin(INTER, HIDDEN), up=lin(INTER, HIDDEN), down=lin(HIDDEN, INTER))
    ones = np.full(HIDDEN, 0x3F80, np.uint16)
    blocks = [Llama4Block(Llama4Attention(*(from_numpy(host[n]) for n in "qkvo"), cfg),
                          Llama4MLP(*(from_numpy(host[n]) for n in ("gate", "up", "down"))), from_numpy(ones), from_numpy(ones),
                          cfg.rms_norm_eps) for _ in range(layers)]
    return Llama4Model(cfg, from_numpy(bf16_bits(rng, (VOCAB, HIDDEN))), blocks, from_numpy(ones), from_numpy(lin(VOCAB, HIDDEN)))


def sync():
    _hip.call("pgk_device_sync")


def window_ms(run, n):
    sync()
    t0 = time.perf_counter()
    for _ in range(n): run()
    sync()
    return (time.perf_counter() - t0) * 1e3 / n


def bench_model(model, ctx, rounds):
    ids = np.random.default_rng(ctx).integers(0, VOCAB, ctx)
    model.init_fixed_cache(ctx)
    model.prefill_fixed_cache(ids[:ctx - 1])
    model.capture_decode()
    tok, pos = int(ids[-1]), ctx - 1
    a = lambda: model.forward(ids)
    b = lambda: model.decode_step(tok, pos)
    c = lambda: model.decode_step_graph(tok, pos)
    for _ in range(2): a()
    for _ in range(10): b(); c()
    na = 3 if ctx >= 2048 else 10
    ta, tb, tc, ta2 = [], [], [], []
    for _ in range(rounds):
        ta.append(window_ms(a, na)); tb.append(window_ms(b, 50)); tc.append(window_ms(c, 50)); ta2.append(window_ms(a, na))
    ma, mb, mc = statistics.median(ta + ta2), statistics.median(tb), statistics.median(tc)
    print(f"model, {len(model.blocks)} layers, context {ctx}, {rounds} rounds (windows of {na} forwards / 50 steps), ms per generated token "
          f"(the captured step has {model._graph.num_nodes} graph nodes):")
    print(f"  (a) forward on the sequence {ma:9.3f} ms   (series a {statistics.median(ta):.3f}, a' {statistics.median(ta2):.3f}, windows {min(ta + ta2):.3f} .. {max(ta + ta2):.3f})")
    print(f"  (b) decode_step            {mb:9.3f} ms   (windows {min(tb):.3f} .. {max(tb):.3f})")
    print(f"  (c) decode_step_graph      {mc:9.3f} ms   (windows {min(tc):.3f} .. {max(tc):.3f})")
    print(f"  b / a {mb / ma:7.4f}   c / a {mc / ma:7.4f}   c / b {mc / mb:7.4f}   a self-spread: a' / a {statistics.median(ta2) / statistics.median(ta):6.4f}", flush=True)


def events_us(run, e0, e1, n=200):
    _hip.call("pgk_event_record", e0, None)
    for _ in range(n): run()
    _hip.call("pgk_event_record", e1, None); _hip.call("pgk_event_sync", e1)
    ms = C.c_float(); _hip.call("pgk_event_elapsed_ms", e0, e1, C.byref(ms))
    return ms.value * 1000 / n


def bench_op(ctx, rounds, e0, e1):
    rng = np.random.default_rng(1)
    q, q2, o = from_numpy(bf16_bits(rng, (HQ, 1, D))), from_numpy(bf16_bits(rng, (HQ, 1, D))), from_numpy(bf16_bits(rng, (HQ, 1, D)))
    k, v = from_numpy(bf16_bits(rng, (HKV, ctx, D))), from_numpy(bf16_bits(rng, (HKV, ctx, D)))
    pos = from_numpy(np.array([ctx - 1], np.int32))
    nbytes = _hip.load().pgk_sdpa_decode_workspace_bytes(HQ, D, ctx)
    ws = from_numpy(np.zeros((nbytes + 3) // 4, np.float32))

    def composition():
        _hip.call("pgk_irope_scale_q", q._p, pos._p, q2._p, 1, HQ, D, C.c_float(0.1), C.c_float(8192.0), PGK_I32, PGK_BF16, None)
        _hip.call("pgk_sdpa_fixed_cache", q2._p, k._p, v._p, o._p, HQ, HKV, 1, ctx, D, C.c_float(0.0), ctx, None, ws._p, PGK_BF16, None)

    def fused():
        _hip.call("pgk_sdpa_irope_fixed_cache", q._p, k._p, v._p, o._p, HQ, HKV, ctx, D, C.c_float(0.1), C.c_float(8192.0), ctx - 1, None,
                  ws._p, PGK_BF16, None)

    for _ in range(20): composition(); fused()
    sync()
    ta, tf, tb = [], [], []
    for _ in range(rounds):
        ta.append(events_us(composition, e0, e1)); tf.append(events_us(fused, e0, e1)); tb.append(events_us(composition, e0, e1))
    ma, mb, mf, mc = statistics.median(ta), statistics.median(tb), statistics.median(tf), statistics.median(ta + tb)
    print(f"op, Hq={HQ} Hkv={HKV} D={D}, context {ctx}, {rounds} rounds of 200 calls:")
    print(f"  irope_scale_q + sdpa_fixed_cache {mc:8.2f} us   (series A {ma:.2f}, A' {mb:.2f}, windows {min(ta + tb):.2f} .. {max(ta + tb):.2f})")
    print(f"  sdpa_irope_fixed_cache           {mf:8.2f} us   (windows {min(tf):.2f} .. {max(tf):.2f})")
    print(f"  new / composition {mf / mc:6.4f}   composition self-spread: A' / A {mb / ma:6.4f}, max / min window {max(ta + tb) / min(ta + tb):6.4f}", flush=True)


def main():
    args = sys.argv[1:]
    rounds, layers = 7, 4
    for flag in ("--rounds", "--layers"):
        if flag in args:
            i = args.index(flag)
            if flag == "--rounds": rounds = int(args[i + 1])
            else: layers = int(args[i + 1])
            del args[i:i + 2]
    contexts = [int(x) for x in args] or [512, 4096]
    _hip.require_device()
    e0, e1 = C.c_void_p(), C.c_void_p()
    _hip.call("pgk_event_create", C.byref(e0)); _hip.call("pgk_event_create", C.byref(e1))
    model = build_model(layers)
    for ctx in contexts:
        bench_model(model, ctx, rounds)
    for ctx in contexts if args else contexts + [16384]:      # 16384: the first of these where Scout's heads take G = 5
        bench_op(ctx, rounds, e0, e1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
