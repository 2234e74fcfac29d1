"""Time decode attention over an FP8 (e4m3) KV cache against the bf16 cache in one process with alternating windows: per round every
variant once, then every variant again (A'), N calls each between device events after a warm-up of all of them.  Prints the median
us per call, the time ratio next to the byte ratio 0.5, the achieved bytes/s of K / V rows, and the spread of each op against itself
(A' / A: the margin inside which two numbers are "the same").  Not a pass / fail gate.  Hq 32, Hkv 8, D 128, bf16.

  (a) decode: sdpa_causal_fixed_cache_fp8 against sdpa_causal_fixed_cache on the same values (the bf16 cache holds the dequantised
      codes) at contexts 512, 4096, 32768 and 131072, the cache as long as the context;
  (b) the quantising writer kv_cache_prefill_gqa_fp8 against kv_cache_prefill_gqa at S = 1 and S = 4096.

usage: attn_kv_fp8_bench.py [--rounds N] [--out FILE] [--sections ab]"""
import argparse, ctypes as C, os, statistics, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from oracle.cpu_ref import fp8_e4m3_table
from pygpukit_amd import _hip
from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import bfloat16
from pygpukit_amd.core.factory import from_numpy

HQ, HKV, D = 32, 8, 128
LINES = []


def say(s=""):
    print(s, flush=True); LINES.append(s)


def bf16(a):
    return from_numpy(np.ascontiguousarray(a, np.float32)).astype(bfloat16)


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
    """-> ({name: median us}, {name: A' / A}): every variant once per round, then every variant again."""
    names = list(variants)
    for k in names: variants[k]()
    _hip.call("pgk_device_sync")
    t, again = {k: [] for k in names}, {k: [] for k in names}
    for _ in range(rounds):
        for k in names: t[k].append(timer.window_us(variants[k], n))
        for k in names: again[k].append(timer.window_us(variants[k], n))
    med = {k: statistics.median(v) for k, v in t.items()}
    return med, {k: statistics.median(again[k]) / med[k] for k in names}


def section_a(timer, rounds):
    from pygpukit_amd.ops.nn import sdpa_causal_fixed_cache, sdpa_causal_fixed_cache_fp8, sdpa_kv_fp8_plan
    rng = np.random.default_rng(0)
    q, out = bf16(rng.standard_normal((HQ, 1, D)) * D ** -0.25), GPUArray((HQ, 1, D), bfloat16)
    for ctx in (512, 4096, 32768, 131072):
        # codes of magnitude 0.25 .. 3.75 with random signs (a block of 4096 rows repeated: the time does not depend on the values)
        kc, vc = (np.tile(rng.integers(0x28, 0x48, (HKV, min(ctx, 4096), D), dtype=np.uint8) | (rng.integers(0, 2, (HKV, min(ctx, 4096), D), dtype=np.uint8) << 7),
                          (1, ctx // min(ctx, 4096), 1)) for _ in range(2))
        k16, v16 = bf16(fp8_e4m3_table()[kc] / 4), bf16(fp8_e4m3_table()[vc] / 4)
        k8, v8, sc = from_numpy(kc), from_numpy(vc), from_numpy(np.full(HKV, 0.25, np.float32))
        med, floor = measure(timer, {"fp8": lambda: sdpa_causal_fixed_cache_fp8(q, k8, v8, sc, sc, out, ctx),
                                     "bf16": lambda: sdpa_causal_fixed_cache(q, k16, v16, out, ctx)}, rounds, 20)
        rows = 2 * HKV * ctx * D
        say(f"(a) decode Hq {HQ} Hkv {HKV} D {D} context {ctx} bfloat16, plan {sdpa_kv_fp8_plan(HQ, HKV, D, ctx, 'bfloat16')}: "
            f"sdpa_causal_fixed_cache_fp8 {med['fp8']:.1f} us ({rows / med['fp8'] / 1e3:.0f} GB/s of K / V codes), sdpa_causal_fixed_cache "
            f"{med['bf16']:.1f} us ({2 * rows / med['bf16'] / 1e3:.0f} GB/s): time ratio {med['fp8'] / med['bf16']:.3f} against the byte ratio 0.500; "
            f"A'/A fp8 {floor['fp8']:.3f}, bf16 {floor['bf16']:.3f}")


def section_b(timer, rounds):
    from pygpukit_amd.ops.basic import kv_cache_prefill_gqa
    from pygpukit_amd.ops.nn import kv_cache_prefill_gqa_fp8
    rng = np.random.default_rng(1)
    cache8, cache16 = from_numpy(np.zeros((HKV, 4096, D), np.uint8)), from_numpy(np.zeros((HKV, 4096, D), np.uint16))
    sc = from_numpy(np.full(HKV, 0.37, np.float32))
    for S in (1, 4096):
        new = bf16(rng.standard_normal((S, HKV, D)))
        med, floor = measure(timer, {"fp8": lambda: kv_cache_prefill_gqa_fp8(new, cache8, sc, 0),
                                     "bf16": lambda: kv_cache_prefill_gqa(new, cache16, HQ, 0)}, rounds, 20)
        n = S * HKV * D
        say(f"(b) writer S {S} Hkv {HKV} D {D} bfloat16: kv_cache_prefill_gqa_fp8 {med['fp8']:.1f} us ({3 * n / med['fp8'] / 1e3:.0f} GB/s read + written), "
            f"kv_cache_prefill_gqa {med['bf16']:.1f} us ({4 * n / med['bf16'] / 1e3:.0f} GB/s): time ratio {med['fp8'] / med['bf16']:.3f}; "
            f"A'/A fp8 {floor['fp8']:.3f}, bf16 {floor['bf16']:.3f}")


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
