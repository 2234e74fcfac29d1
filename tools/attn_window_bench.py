"""Time sliding-window attention against causal attention in one process with alternating windows: per round every variant of a
section once, then the first variant again (A'), N calls each between device events after a warm-up of all of them.  Prints the
median us per call, the time ratio next to the ratio of live work, and the spread of the first variant against itself (A' / A:
the margin inside which two numbers are "the same").  Not a pass / fail gate.  Mistral-7B's shape: Hq 32, Hkv 8, D 128, W 4096, bf16.

  (a) prefill: sdpa_sliding_window against sdpa_causal on the same tensors at S = 8192 and 16384; the band walk should approach
      the live-tile ratio (S W - W^2 / 2) / (S^2 / 2) = 0.75 and 0.44;
  (b) decode: sdpa_sliding_window_fixed_cache over a linear cache of 32768 rows and over a ring of W rows against
      sdpa_causal_fixed_cache, all at context 32768; the window split should approach W / ctx = 0.125.

usage: attn_window_bench.py [--rounds N] [--out FILE] [--sections ab]"""
import argparse, ctypes as C, os, statistics, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from pygpukit_amd import _hip
from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import bfloat16
from pygpukit_amd.core.factory import from_numpy

HQ, HKV, D, W = 32, 8, 128, 4096
LINES = []


def say(s=""):
    print(s, flush=True); LINES.append(s)


def bf16(rng, shape, std=1.0):
    return from_numpy(std * rng.standard_normal(shape, dtype=np.float32)).astype(bfloat16)


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
    from pygpukit_amd.ops.nn import sdpa_causal, sdpa_sliding_window, sdpa_window_plan
    rng = np.random.default_rng(0)
    for S in (8192, 16384):
        q = bf16(rng, (HQ, S, D), D ** -0.25)
        k, v = bf16(rng, (HKV, S, D), D ** -0.25), bf16(rng, (HKV, S, D))
        out = GPUArray((HQ, S, D), bfloat16)
        med, floor, lo, hi = measure(timer, {"window": lambda: sdpa_sliding_window(q, k, v, W, out=out),
                                             "causal": lambda: sdpa_causal(q, k, v, out=out)}, rounds, 3)
        live = (S * W - W * W / 2) / (S * S / 2)
        flops = 4.0 * HQ * D * (S * W - W * W / 2)
        say(f"(a) prefill Hq {HQ} Hkv {HKV} D {D} W {W} S {S} bfloat16, plan {sdpa_window_plan(HQ, HKV, S, S, D, W, 'bfloat16')}: "
            f"sdpa_sliding_window {med['window']:.0f} us ({flops / med['window'] / 1e6:.0f} TFLOP/s of live work), sdpa_causal {med['causal']:.0f} us: "
            f"time ratio {med['window'] / med['causal']:.3f} against the live-tile ratio {live:.3f}; A'/A {floor:.3f}, windows {lo:.0f}..{hi:.0f} us")


def section_b(timer, rounds):
    from pygpukit_amd.ops.nn import sdpa_causal_fixed_cache, sdpa_sliding_window_fixed_cache
    rng = np.random.default_rng(1)
    ctx = 32768
    q, out = bf16(rng, (HQ, 1, D), D ** -0.25), GPUArray((HQ, 1, D), bfloat16)
    kl, vl = bf16(rng, (HKV, ctx, D), D ** -0.25), bf16(rng, (HKV, ctx, D))
    kr, vr = bf16(rng, (HKV, W, D), D ** -0.25), bf16(rng, (HKV, W, D))
    med, floor, lo, hi = measure(timer, {"linear": lambda: sdpa_sliding_window_fixed_cache(q, kl, vl, out, ctx, W),
                                         "ring": lambda: sdpa_sliding_window_fixed_cache(q, kr, vr, out, ctx, W, ring=True),
                                         "causal": lambda: sdpa_causal_fixed_cache(q, kl, vl, out, ctx)}, rounds, 20)
    say(f"(b) decode Hq {HQ} Hkv {HKV} D {D} W {W} context {ctx} bfloat16: sdpa_sliding_window_fixed_cache over a linear cache of {ctx} rows "
        f"{med['linear']:.1f} us, over a ring of {W} rows {med['ring']:.1f} us, sdpa_causal_fixed_cache {med['causal']:.1f} us: time ratios "
        f"{med['linear'] / med['causal']:.3f} (linear) and {med['ring'] / med['causal']:.3f} (ring) against W / ctx = {W / ctx:.3f}; "
        f"{2 * HKV * W * D * 2 / med['linear'] / 1e3:.0f} GB/s of live K / V rows (linear); A'/A {floor:.3f}, windows {lo:.1f}..{hi:.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sections", default="ab")
    a = ap.parse_args()
    timer = Timer()
    for s, fn in (("a", section_a), ("b", section_b)):
        if s in a.sections:
            fn(timer, a.rounds)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
