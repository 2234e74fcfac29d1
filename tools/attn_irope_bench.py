"""Time pgk_sdpa_irope against pgk_sdpa_causal on the same tensors, in one process, alternating: per round
causal (A), irope, causal again (A'), 20 launches each between device events after a warm-up of both ops.  Prints the
median time of each series, irope / causal, and the spread of sdpa_causal against itself (median A' / median A and the
min..max of all causal windows) - the margin inside which the ratio means "the same".
Positions are 0..S-1 with the default scales (attn_scale 0.1, floor_scale 8192) and offset 0, i.e. the model's call;
TFLOP/s = 4 S^2 D Hq / 2 per launch.
usage: attn_irope_bench.py [--rounds N] [Hq Hkv S ...]     (default: 40 8 4096  40 8 2048, the Llama-4 Scout heads; D = 128)"""
import ctypes as C, os, statistics, sys, numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from pygpukit_amd import _hip
D = 128
PGK_BF16, PGK_I64 = 3, 4      # pgk_dtype, include/pgk_hip.h


def setup(hq, hkv, S):
    rng = np.random.default_rng(0)
    def dev(arr):
        p = C.c_void_p(); _hip.call("pgk_malloc", C.byref(p), arr.nbytes)
        _hip.call("pgk_memcpy_h2d", p, arr.ctypes.data_as(C.c_void_p), arr.nbytes, None); return p
    bf = lambda shape: (rng.standard_normal(shape).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    q, k, v = dev(bf((S, hq, D))), dev(bf((hkv, S, D))), dev(bf((hkv, S, D)))
    pos = dev(np.arange(S, dtype=np.int64))
    o = C.c_void_p(); _hip.call("pgk_malloc", C.byref(o), S * hq * D * 2)
    # q/out in the projection's [S, H, D] layout, K/V in the cache layout [Hkv, S, D]
    causal = lambda: _hip.call("pgk_sdpa_causal", q, k, v, o, hq, hkv, S, S, D, C.c_float(0.0), D, hq * D, S * D, D, D, hq * D, PGK_BF16, None)
    irope = lambda: _hip.call("pgk_sdpa_irope", q, k, v, pos, o, hq, hkv, S, S, D, C.c_float(0.1), C.c_float(8192.0), 0,
                              D, hq * D, S * D, D, D, hq * D, PGK_I64, PGK_BF16, None)
    return causal, irope


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
    a = [int(x) for x in args] or [40, 8, 4096, 40, 8, 2048]
    _hip.require_device()
    e0, e1 = C.c_void_p(), C.c_void_p()
    _hip.call("pgk_event_create", C.byref(e0)); _hip.call("pgk_event_create", C.byref(e1))
    for i in range(0, len(a), 3):
        hq, hkv, S = a[i:i + 3]
        causal, irope = setup(hq, hkv, S)
        for _ in range(5): causal(); irope()
        _hip.call("pgk_device_sync")
        ta, ti, tb = [], [], []
        for _ in range(rounds):
            ta.append(window_us(causal, e0, e1)); ti.append(window_us(irope, e0, e1)); tb.append(window_us(causal, e0, e1))
        ma, mi, mb = statistics.median(ta), statistics.median(ti), statistics.median(tb)
        mc = statistics.median(ta + tb)
        flop = 4.0 * S * S * D * hq / 2
        print(f"Hq={hq} Hkv={hkv} S={S} D={D}, {rounds} rounds of 20 launches:")
        print(f"  sdpa_causal  {mc:9.1f} us {flop / mc / 1e6:7.1f} TFLOP/s   (series A {ma:.1f} us, series A' {mb:.1f} us, windows {min(ta + tb):.1f} .. {max(ta + tb):.1f} us)")
        print(f"  sdpa_irope   {mi:9.1f} us {flop / mi / 1e6:7.1f} TFLOP/s   (windows {min(ti):.1f} .. {max(ti):.1f} us)")
        print(f"  irope / causal time ratio {mi / mc:6.4f}   causal self-spread: A' / A {mb / ma:6.4f}, max / min window {max(ta + tb) / min(ta + tb):6.4f}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
