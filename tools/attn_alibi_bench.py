"""Time the ALiBi attention kernels against the causal ones on the same tensors, in one process, alternating: per round
causal (A), alibi, causal again (A'), 20 launches each between device events after a warm-up of both ops.  Prints the median
time of each series, alibi / causal, and the spread of the causal op against itself (median A' / median A and the min..max
of all causal windows) - the margin inside which the ratio means "the same".
  prefill: pgk_sdpa_alibi against pgk_sdpa_causal, q/out in [S, H, D], K/V in [Hkv, S, D]; TFLOP/s = 4 S^2 D Hq / 2
  decode:  pgk_sdpa_alibi_fixed_cache against pgk_sdpa_fixed_cache, one query row over a FULL cache of `rows` rows; GB/s of
           K and V read once
Slopes are alibi_init_slopes(Hq); D = 128, bf16.
usage: attn_alibi_bench.py [--rounds N] [prefill Hq Hkv S | decode Hq Hkv rows] ...
default: prefill 32 32 2048  prefill 32 32 4096  prefill 32 8 4096  decode 32 32 512  decode 32 32 4096  decode 32 32 16384"""
import ctypes as C, os, statistics, sys, numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from pygpukit_amd import _hip
D = 128
PGK_BF16 = 3      # pgk_dtype, include/pgk_hip.h
DEFAULT = "prefill 32 32 2048 prefill 32 32 4096 prefill 32 8 4096 decode 32 32 512 decode 32 32 4096 decode 32 32 16384".split()


def dev(arr):
    p = C.c_void_p(); _hip.call("pgk_malloc", C.byref(p), arr.nbytes)
    _hip.call("pgk_memcpy_h2d", p, arr.ctypes.data_as(C.c_void_p), arr.nbytes, None); return p


def bf(rng, shape):
    return (rng.standard_normal(shape).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


def slopes(hq):
    return dev(np.array([2 ** (-8 * (h + 1) / hq) for h in range(hq)], np.float32))


def setup_prefill(hq, hkv, S):
    rng = np.random.default_rng(0)
    q, k, v, sl = dev(bf(rng, (S, hq, D))), dev(bf(rng, (hkv, S, D))), dev(bf(rng, (hkv, S, D))), slopes(hq)
    o = C.c_void_p(); _hip.call("pgk_malloc", C.byref(o), S * hq * D * 2)
    causal = lambda: _hip.call("pgk_sdpa_causal", q, k, v, o, hq, hkv, S, S, D, C.c_float(0.0), D, hq * D, S * D, D, D, hq * D, PGK_BF16, None)
    alibi = lambda: _hip.call("pgk_sdpa_alibi", q, k, v, sl, o, hq, hkv, S, S, D, C.c_float(0.0), D, hq * D, S * D, D, D, hq * D, PGK_BF16, None)
    return causal, alibi


def setup_decode(hq, hkv, rows):
    rng = np.random.default_rng(0)
    q, k, v, sl = dev(bf(rng, (hq, 1, D))), dev(bf(rng, (hkv, rows, D))), dev(bf(rng, (hkv, rows, D))), slopes(hq)
    o = C.c_void_p(); _hip.call("pgk_malloc", C.byref(o), hq * D * 2)
    ws = C.c_void_p(); _hip.call("pgk_malloc", C.byref(ws), _hip.load().pgk_sdpa_decode_workspace_bytes(hq, D, rows))
    causal = lambda: _hip.call("pgk_sdpa_fixed_cache", q, k, v, o, hq, hkv, 1, rows, D, C.c_float(0.0), rows, None, ws, PGK_BF16, None)
    alibi = lambda: _hip.call("pgk_sdpa_alibi_fixed_cache", q, k, v, sl, o, hq, hkv, 1, rows, D, C.c_float(0.0), rows, None, ws, PGK_BF16, None)
    return causal, alibi


def window_us(run, e0, e1, n=20):
    _hip.call("pgk_event_record", e0, None)
    for _ in range(n): run()
    _hip.call("pgk_event_record", e1, None); _hip.call("pgk_event_sync", e1)
    ms = C.c_float(); _hip.call("pgk_event_elapsed_ms", e0, e1, C.byref(ms))
    return ms.value * 1000 / n


def main():
    args = sys.argv[1:]
    rounds = 15
    if "--rounds" in args:
        i = args.index("--rounds"); rounds = int(args[i + 1]); del args[i:i + 2]
    a = args or DEFAULT
    _hip.require_device()
    e0, e1 = C.c_void_p(), C.c_void_p()
    _hip.call("pgk_event_create", C.byref(e0)); _hip.call("pgk_event_create", C.byref(e1))
    for i in range(0, len(a), 4):
        kind, (hq, hkv, n) = a[i], (int(x) for x in a[i + 1:i + 4])
        causal, alibi = (setup_prefill if kind == "prefill" else setup_decode)(hq, hkv, n)
        for _ in range(5): causal(); alibi()
        _hip.call("pgk_device_sync")
        ta, ti, tb = [], [], []
        for _ in range(rounds):
            ta.append(window_us(causal, e0, e1)); ti.append(window_us(alibi, e0, e1)); tb.append(window_us(causal, e0, e1))
        ma, mi, mb = statistics.median(ta), statistics.median(ti), statistics.median(tb)
        mc = statistics.median(ta + tb)
        if kind == "prefill":
            work, unit, names = 4.0 * n * n * D * hq / 2 / 1e6, "TFLOP/s", ("sdpa_causal", "sdpa_alibi")
            print(f"prefill Hq={hq} Hkv={hkv} S={n} D={D}, {rounds} rounds of 20 launches:")
        else:
            work, unit, names = 2.0 * hkv * n * D * 2 / 1e3, "GB/s", ("sdpa_causal_fixed_cache", "sdpa_alibi_fixed_cache")
            print(f"decode Hq={hq} Hkv={hkv} cache and context {n} rows D={D}, {rounds} rounds of 20 launches:")
        print(f"  {names[0]:24s} {mc:9.1f} us {work / mc:8.1f} {unit}   (series A {ma:.1f} us, series A' {mb:.1f} us, windows {min(ta + tb):.1f} .. {max(ta + tb):.1f} us)")
        print(f"  {names[1]:24s} {mi:9.1f} us {work / mi:8.1f} {unit}   (windows {min(ti):.1f} .. {max(ti):.1f} us)")
        print(f"  alibi / causal time ratio {mi / mc:6.4f}   causal self-spread: A' / A {mb / ma:6.4f}, max / min window {max(ta + tb) / min(ta + tb):6.4f}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
