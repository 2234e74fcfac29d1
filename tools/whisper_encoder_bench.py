"""Time the Whisper-encoder ops against what the project could run before them, in one process with alternating windows: per
round A (new), B (old), A' (new again), N calls each between device events after a warm-up of all of them.  Prints medians,
old / new, and the new call against itself (A' / A and min..max of its windows: the margin inside which two numbers are "the
same").  Every comparison first checks that both sides compute the same thing (rel_err).

  (a) conv1d (one launch, weights pre-packed) against the composition of existing ops: transpose to [L, C], copy into a
      zero-bordered buffer, (stride 2: split even / odd positions,) copy the K shifted row windows side by side, transpose to the
      im2col matrix [L_out, K C], matmul_nt, bias_add_inplace, gelu, and a transpose back to [C_out, L_out] (stem 1) or the
      position add (stem 2).  Whisper-large stem: [1,128,3000] -> 1280, K=3 and [1,1280,3000] -> 1280, K=3, stride 2; bf16, float32.
  (b) sdpa_noncausal against sdpa_causal on the same tensors, H=20, S=1500, D=64, bf16: about twice the tiles are live; the
      TFLOP/s count all S^2 scores (4 H S^2 D flop) for the non-causal call and half of that for the causal one.
  (c) one encoder layer at d_model=1280, 20 heads, S=1500, bf16: WhisperEncoderLayer against the reference-style path with this
      project's ops - separate q / k / v GEMMs, [S,H,D] -> [H,S,D] transposes, batched_matmul -> softmax -> batched_matmul with
      the [H,S,S] scores in memory, transpose back, out_proj, fc1 + gelu, fc2 (1/sqrt(D) folded into the q weights).
usage: whisper_encoder_bench.py [--rounds N]"""
import ctypes as C, os, statistics, sys, numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from pygpukit_amd import _hip, ops
from pygpukit_amd.asr.whisper import WhisperConfig, WhisperEncoderLayer
from pygpukit_amd.core import GPUArray, bfloat16, float32, from_numpy, zeros
from pygpukit_amd.ops.conv import conv1d, conv1d_pack_weight
from pygpukit_amd.ops.elementwise import copy_to


def dev(a, dt):
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


def compare(name, new, old, e0, e1, rounds, n, flop_new=None, flop_old=None):
    for _ in range(3): new(); old()
    _hip.call("pgk_device_sync")
    ta, tb, to = [], [], []
    for _ in range(rounds):
        ta.append(window_us(new, e0, e1, n)); to.append(window_us(old, e0, e1, n)); tb.append(window_us(new, e0, e1, n))
    _hip.call("pgk_device_sync")
    med = statistics.median
    mn, mo = med(ta + tb), med(to)
    tf = f"  new {flop_new / mn / 1e6:6.1f} TFLOP/s" if flop_new else ""
    tf += f"  old {flop_old / mo / 1e6:6.1f} TFLOP/s" if flop_old else ""
    print(f"{name}: new {mn:9.1f} us  old {mo:9.1f} us  old / new {mo / mn:6.3f}{tf}   (new against itself: A'/A {med(tb) / med(ta):6.4f}, "
          f"windows {min(ta + tb):.1f} .. {max(ta + tb):.1f} us; old windows {min(to):.1f} .. {max(to):.1f} us)", flush=True)


def conv_pair(c_in, c_out, length, stride, dt, second):
    """-> (new(), old()) for one stem convolution; second: stride-2 conv with channels-last output and position add."""
    rng = np.random.default_rng(1)
    K, pad = 3, 1
    l_out = (length + 2 * pad - K) // stride + 1
    w_np = rng.standard_normal((c_out, c_in, K)) / np.sqrt(c_in * K)
    x, w, b = dev(rng.standard_normal((1, c_in, length)), dt), dev(w_np, dt), dev(0.1 * rng.standard_normal(c_out), dt)
    pos = dev(0.1 * rng.standard_normal((l_out, c_out)), dt) if second else None
    packed = conv1d_pack_weight(w) if dt != float32 else None
    out_new = GPUArray((1, l_out, c_out) if second else (1, c_out, l_out), dt)

    def new():
        return conv1d(x, w, b, stride, pad, activation="gelu", channels_last_out=second, add=pos, packed_weight=packed, out=out_new)

    wcat = dev(w_np.transpose(0, 2, 1).reshape(c_out, K * c_in), dt)              # [C_out, (t, c)]
    x2 = x._view(0, (c_in, length))
    padded = zeros((length + 2 * pad, c_in), dt)                                   # the borders stay zero
    stack = GPUArray((K, l_out, c_in), dt)
    half = (length + 2 * pad) // 2

    def old():
        copy_to(ops.transpose(x2), padded._view(pad * c_in, (length, c_in)))
        if stride == 1:
            taps = [padded._view(t * c_in, (l_out, c_in)) for t in range(K)]
        else:
            eo = ops.transpose_3d_021(padded.view((half, 2, c_in)))               # [even | odd positions][half][C]
            taps = [eo._view(0, (l_out, c_in)), eo._view(half * c_in, (l_out, c_in)), eo._view(c_in, (l_out, c_in))]
        for t in range(K):
            copy_to(taps[t], stack._view(t * l_out * c_in, (l_out, c_in)))
        col = ops.transpose_3d_021(stack).view((l_out, K * c_in))                # im2col, one row per output position
        y = ops.matmul_nt(col, wcat)
        ops.bias_add_inplace(y, b)
        ops.gelu(y, out=y)
        return ops.add(y, pos, out=y) if second else ops.transpose(y)

    assert stride == 1 or (length + 2 * pad) % 2 == 0
    err = rel(new(), old())
    assert err < (1e-5 if dt == float32 else 1e-2), err
    return new, old, 2.0 * c_out * c_in * K * l_out, err


def attention_pair(H, S, D, dt):
    rng = np.random.default_rng(2)
    q, k, v = (dev(rng.standard_normal((H, S, D)), dt) for _ in range(3))
    o1, o2 = GPUArray((H, S, D), dt), GPUArray((H, S, D), dt)
    return (lambda: ops.sdpa_noncausal(q, k, v, out=o1)), (lambda: ops.sdpa_causal(q, k, v, out=o2)), 4.0 * H * S * S * D


def layer_pair(d, heads, S, dt):
    rng = np.random.default_rng(3)
    ffn, hd = 4 * d, d // heads
    mat = lambda r, c: (rng.standard_normal((r, c)) / np.sqrt(c)).astype(np.float32)
    vec = lambda n, m=0.0: (m + 0.1 * rng.standard_normal(n)).astype(np.float32)
    w = {"self_attn_k_bias": None}
    for n in "qkv":
        w[f"self_attn_{n}_weight"] = mat(d, d)
    w.update(self_attn_q_bias=vec(d), self_attn_v_bias=vec(d), self_attn_out_weight=mat(d, d), self_attn_out_bias=vec(d),
             self_attn_layer_norm_weight=vec(d, 1.0), self_attn_layer_norm_bias=vec(d), fc1_weight=mat(ffn, d), fc1_bias=vec(ffn),
             fc2_weight=mat(d, ffn), fc2_bias=vec(d), final_layer_norm_weight=vec(d, 1.0), final_layer_norm_bias=vec(d))
    layer = WhisperEncoderLayer(WhisperConfig(d_model=d, encoder_attention_heads=heads, encoder_ffn_dim=ffn), w, dt)
    x = dev(rng.standard_normal((S, d)), dt)
    g = {k2: dev(v2, dt) for k2, v2 in w.items() if v2 is not None}
    g["self_attn_k_bias"] = dev(np.zeros(d), dt)
    scale = 1.0 / np.sqrt(hd)
    g["self_attn_q_weight"], g["self_attn_q_bias"] = dev(w["self_attn_q_weight"] * scale, dt), dev(w["self_attn_q_bias"] * scale, dt)

    def heads_first(a):
        return ops.transpose_3d_021(a.view((S, heads, hd)))                      # [H, S, D]

    def old():
        h = ops.layernorm(x, g["self_attn_layer_norm_weight"], g["self_attn_layer_norm_bias"])
        q, k, v = (heads_first(ops.matmul_nt(h, g[f"self_attn_{n}_weight"], g[f"self_attn_{n}_bias"])) for n in "qkv")
        p = ops.softmax(ops.batched_matmul(q, ops.transpose_3d_012(k)))           # [H, S, S] in memory
        a = ops.transpose_3d_021(ops.batched_matmul(p, v)).view((S, d))
        y = ops.add(x, ops.matmul_nt(a, g["self_attn_out_weight"], g["self_attn_out_bias"]))
        h = ops.layernorm(y, g["final_layer_norm_weight"], g["final_layer_norm_bias"])
        f = ops.matmul_nt(h, g["fc1_weight"], g["fc1_bias"])
        ops.gelu(f, out=f)
        return ops.add(y, ops.matmul_nt(f, g["fc2_weight"], g["fc2_bias"]))

    err = rel(layer(x), old())
    assert err < 2e-2, err
    return (lambda: layer(x)), old, err


def main():
    args = sys.argv[1:]
    rounds = 9
    if "--rounds" in args:
        i = args.index("--rounds"); rounds = int(args[i + 1])
    _hip.require_device()
    e0, e1 = C.c_void_p(), C.c_void_p()
    _hip.call("pgk_event_create", C.byref(e0)); _hip.call("pgk_event_create", C.byref(e1))
    for dt, name in ((bfloat16, "bf16"), (float32, "float32")):
        for c_in, stride, second in ((128, 1, False), (1280, 2, True)):
            new, old, flop, err = conv_pair(c_in, 1280, 3000, stride, dt, second)
            compare(f"(a) conv1d [1,{c_in},3000]->1280 K=3 stride {stride} {name} (+gelu{', channels-last, +pos' if second else ''}; old vs new rel_err {err:.1e})",
                    new, old, e0, e1, rounds, 10, flop, flop)
    new, old, flop = attention_pair(20, 1500, 64, bfloat16)
    compare("(b) sdpa_noncausal (new) vs sdpa_causal (old) H=20 S=1500 D=64 bf16", new, old, e0, e1, rounds, 20, flop, flop / 2)
    new, old, err = layer_pair(1280, 20, 1500, bfloat16)
    compare(f"(c) encoder layer d_model=1280 H=20 S=1500 bf16 (old vs new rel_err {err:.1e})", new, old, e0, e1, rounds, 5)
    return 0


if __name__ == "__main__":
    sys.exit(main())
