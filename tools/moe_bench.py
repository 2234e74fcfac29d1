"""Time the Mixture-of-Experts path: the whole MoELayer forward and its two grouped expert GEMMs alone, at the Mixtral-8x7B
and Qwen3-30B-A3B shapes, bf16 and fp8 experts, T tokens in {1, 8, 64, 512, 4096}; beside them, the same FLOPs as E
dense bf16 pgk_gemm_nt calls of M = ceil(T*k/E) rows (one per expert weight).
usage: moe_bench.py [mixtral|qwen3 ...]
Each figure: median of 5 device-event windows of n calls each, after 3 warm-up calls.
  active bytes = distinct experts routed to x expert weight bytes (gate, up, down codes + block scales)
  FLOP         = 2 * T * k * 3 * H * I   (gate + up + down)
  GB/s         = active bytes / grouped-GEMM time;  TFLOP/s = FLOP / time."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pygpukit_amd import _hip  # noqa: E402
from pygpukit_amd.core.array import GPUArray  # noqa: E402
from pygpukit_amd.core.dtypes import bfloat16, int32, uint8  # noqa: E402
from pygpukit_amd.llm.config import TransformerConfig  # noqa: E402
from pygpukit_amd.llm.layers import LinearFP8, MoELayer  # noqa: E402
from pygpukit_amd.ops import grouped_gemm_bf16, grouped_gemm_fp8_bf16, moe_compute_permutation, moe_topk_softmax  # noqa: E402
from pygpukit_amd.ops.nn.fused import glu_packed  # noqa: E402

SHAPES = {"mixtral": dict(H=4096, I=14336, E=8, k=2), "qwen3": dict(H=2048, I=768, E=128, k=8)}
TOKENS = (1, 8, 64, 512, 4096)
PGK_BF16 = 3


def fill_random(arr: GPUArray, seed: int, bf16_values: bool) -> None:
    """A 16 MiB random block repeated over the array (device copies): realistic bit patterns without gigabytes of host RNG."""
    rng = np.random.default_rng(seed)
    n = min(arr.nbytes, 16 << 20)
    if bf16_values:
        blk = ((rng.standard_normal(n // 2).astype(np.float32) * 0.02).view(np.uint32) >> 16).astype(np.uint16).view(np.uint8)
    else:   # e4m3 codes with exponent fields 5..9 (no NaN codes)
        blk = (rng.integers(0, 2, n) << 7 | rng.integers(5, 10, n) << 3 | rng.integers(0, 8, n)).astype(np.uint8)
    _hip.call("pgk_memcpy_h2d", arr._p, blk.ctypes.data_as(C.c_void_p), n, None)
    off = n
    while off < arr.nbytes:
        m = min(off, arr.nbytes - off)
        _hip.call("pgk_memcpy_d2d", C.c_void_p(arr.device_ptr + off), arr._p, m, None)
        off += m


def scales(shape, seed):
    s = np.exp2(np.random.default_rng(seed).integers(-13, -10, shape)).astype(np.float32)
    a = GPUArray(shape, bfloat16)
    a.copy_from_numpy((s.view(np.uint32) >> 16).astype(np.uint16))
    return a


def timed(fn, n):
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        _hip.call("pgk_event_create", C.byref(e))
    for _ in range(3):
        fn()
    ms = []
    for _ in range(5):
        _hip.call("pgk_event_record", ev[0], None)
        for _ in range(n):
            fn()
        _hip.call("pgk_event_record", ev[1], None)
        _hip.call("pgk_event_sync", ev[1])
        t = C.c_float()
        _hip.call("pgk_event_elapsed_ms", ev[0], ev[1], C.byref(t))
        ms.append(t.value / n)
    for e in ev:
        _hip.call("pgk_event_destroy", e)
    return float(np.median(ms)) * 1e3      # us


def bench(name, fp8):
    s = SHAPES[name]
    H, I, E, k = s["H"], s["I"], s["E"], s["k"]
    wdt = uint8 if fp8 else bfloat16
    wgu, wd = GPUArray((E, 2 * I, H), wdt), GPUArray((E, H, I), wdt)
    fill_random(wgu, 1, not fp8)
    fill_random(wd, 2, not fp8)
    sgu = scales((E, 2 * I // 128, H // 128), 3) if fp8 else None
    sd = scales((E, H // 128, I // 128), 4) if fp8 else None
    per_expert = 3 * H * I * (1 if fp8 else 2) + (3 * (H // 128) * (I // 128) * 2 if fp8 else 0)

    def view(a, e, j, rows):                    # rows j*rows .. of expert e, as a 2-D view
        return a._view(e * a.shape[1] * a.shape[2] + j * rows * a.shape[2], (rows, a.shape[2]))

    experts = []
    for e in range(E):
        g, u, d = view(wgu, e, 0, I), view(wgu, e, 1, I), view(wd, e, 0, H)
        if fp8:
            experts.append((LinearFP8(g, view(sgu, e, 0, I // 128)), LinearFP8(u, view(sgu, e, 1, I // 128)),
                            LinearFP8(d, view(sd, e, 0, H // 128))))
        else:
            experts.append((g, u, d))
    router = GPUArray((E, H), bfloat16)
    fill_random(router, 5, True)
    cfg = TransformerConfig(hidden_size=H, num_heads=16, num_layers=1, intermediate_size=I, num_experts=E,
                            num_experts_per_tok=k, moe_intermediate_size=I)
    layer = MoELayer(cfg, router, experts)
    gemm = grouped_gemm_fp8_bf16 if fp8 else grouped_gemm_bf16
    wargs = (lambda w, sc: (w, sc)) if fp8 else (lambda w, sc: (w,))
    for T in TOKENS:
        x = GPUArray((T, H), bfloat16)
        fill_random(x, 10 + T, True)
        n = 20 if T <= 64 else 5
        t_layer = timed(lambda: layer(x), n)
        logits = layer.gate(x)
        w, idx = GPUArray((T, k), bfloat16), GPUArray((T, k), int32)
        moe_topk_softmax(logits, w, idx, k)
        counts, offsets = GPUArray((E,), int32), GPUArray((E + 1,), int32)
        perm, rev = GPUArray((T * k,), int32), GPUArray((T * k,), int32)
        tiles = moe_compute_permutation(idx, counts, offsets, perm, rev, E, k)
        act = glu_packed(gemm(x, *wargs(layer.w_gate_up, layer.s_gate_up), None, tiles=tiles, expert_offsets=offsets,
                              permute_indices=perm, top_k=k), I)
        t_gu = timed(lambda: gemm(x, *wargs(layer.w_gate_up, layer.s_gate_up), None, tiles=tiles, expert_offsets=offsets,
                                  permute_indices=perm, top_k=k), n)
        t_dn = timed(lambda: gemm(act, *wargs(layer.w_down, layer.s_down), None, tiles=tiles, expert_offsets=offsets,
                                  out_slabs=True), n)
        active = int((counts.to_numpy() > 0).sum())
        flop = 6.0 * T * k * H * I
        t_g = t_gu + t_dn
        line = (f"{name:7s} {'fp8 ' if fp8 else 'bf16'} T={T:5d} active={active:3d}  layer {t_layer:9.1f} us  grouped {t_g:9.1f} us "
                f"(gate_up {t_gu:8.1f} + down {t_dn:8.1f})  {active * per_expert / t_g / 1e3:7.0f} GB/s  "
                f"{flop / t_g / 1e6:7.1f} TFLOP/s")
        if not fp8:     # the dense bf16 GEMMs of equal FLOPs: E x (gate_up + down) at M = ceil(T*k/E)
            M = max(1, -(-T * k // E))
            a = GPUArray((M, H), bfloat16)
            fill_random(a, 7, True)
            a2 = GPUArray((M, I), bfloat16)
            fill_random(a2, 8, True)
            cgu, cd = GPUArray((M, 2 * I), bfloat16), GPUArray((M, H), bfloat16)

            def dense():
                for e in range(E):
                    _hip.call("pgk_gemm_nt", a._p, view(wgu, e, 0, 2 * I)._p, None, cgu._p, M, 2 * I, H, PGK_BF16, None)
                    _hip.call("pgk_gemm_nt", a2._p, view(wd, e, 0, H)._p, None, cd._p, M, H, I, PGK_BF16, None)
            t_dense = timed(dense, max(1, n // 4))
            line += f"  | dense M={M:4d} x{E}: {t_dense:9.1f} us {6.0 * M * E * H * I / t_dense / 1e6:7.1f} TFLOP/s"
        print(line, flush=True)


def main():
    _hip.require_device()
    names = sys.argv[1:] or list(SHAPES)
    for name in names:
        for fp8 in (False, True):
            bench(name, fp8)


if __name__ == "__main__":
    main()
