"""Time pgk_sdpa_causal_fp8 against pgk_sdpa_causal (prefill) in the same run: TFLOP/s = 4 S^2 D Hq / 2 per launch, three
warm-up and ten timed launches each (as tools/attn_bench.py), and the fp8 / bf16 ratio.  Then one
`rocprofv3 --kernel-trace --stats` run per shape of the fp8 op alone (a fresh child process) gives the share of its launch spent
in the two quantisation pre-passes.
usage: attn_fp8_bench.py [--no-profile] [Hq Hkv S ...]     (default: 32 8 4096  16 8 2048; D = 128)"""
import csv, ctypes as C, glob, os, signal, subprocess, sys, tempfile, numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
from pygpukit_amd import _hip
D = 128
PGK_BF16 = 3      # pgk_dtype, include/pgk_hip.h


def setup(hq, hkv, S):
    rng = np.random.default_rng(0)
    def dev(arr):
        p = C.c_void_p(); _hip.call("pgk_malloc", C.byref(p), arr.nbytes)
        _hip.call("pgk_memcpy_h2d", p, arr.ctypes.data_as(C.c_void_p), arr.nbytes, None); return p
    bf = lambda shape: (rng.standard_normal(shape).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    q, k, v = dev(bf((S, hq, D))), dev(bf((hkv, S, D))), dev(bf((hkv, S, D)))
    o = C.c_void_p(); _hip.call("pgk_malloc", C.byref(o), S * hq * D * 2)
    # q/out in the projection's [S, H, D] layout, K/V in the cache layout [Hkv, S, D]
    return lambda name: _hip.call(name, q, k, v, o, hq, hkv, S, S, D, C.c_float(0.0), D, hq * D, S * D, D, D, hq * D, PGK_BF16, None)


def time_us(run, name):
    e0, e1 = C.c_void_p(), C.c_void_p()
    _hip.call("pgk_event_create", C.byref(e0)); _hip.call("pgk_event_create", C.byref(e1))
    for _ in range(3): run(name)
    _hip.call("pgk_event_record", e0, None)
    for _ in range(10): run(name)
    _hip.call("pgk_event_record", e1, None); _hip.call("pgk_event_sync", e1)
    ms = C.c_float(); _hip.call("pgk_event_elapsed_ms", e0, e1, C.byref(ms))
    return ms.value * 100


def child(hq, hkv, S):
    """the profiled workload: the fp8 op alone"""
    _hip.require_device()
    run = setup(hq, hkv, S)
    for _ in range(13): run("pgk_sdpa_causal_fp8")
    _hip.call("pgk_device_sync")


def profile(hq, hkv, S):
    with tempfile.TemporaryDirectory() as out:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--",
               sys.executable, os.path.abspath(__file__), "--child", str(hq), str(hkv), str(S)]
        # its own session: on a time-out the whole group goes, rocprofv3 AND the Python child that holds the GPU
        proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, start_new_session=True)
        try:
            log, _ = proc.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            os.killpg(proc.pid, signal.SIGKILL)
            log, _ = proc.communicate()
            print(f"rocprofv3 run timed out:\n{log[-2000:]}", flush=True)
            return 1
        files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
        if proc.returncode != 0 or not files:
            print(f"rocprofv3 run failed (exit {proc.returncode}):\n{log[-2000:]}", flush=True)
            return 1
        rows = list(csv.DictReader(open(files[0])))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    print(f"rocprofv3 --kernel-trace --stats, pgk_sdpa_causal_fp8 alone, Hq={hq} Hkv={hkv} S={S} (13 launches):")
    share = 0.0
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        name = r["Name"].split("(")[0].replace("void ", "")
        t = float(r["TotalDurationNs"])
        print(f"  {name:<55s} {int(r['Calls']):4d} calls {float(r['AverageNs']) / 1e3:9.1f} us avg {100 * t / total:6.2f} %")
        if "fp8_head_" in name: share += t / total
    print(f"  quantisation pre-passes (fp8_head_absmax_kernel + fp8_head_codes_kernel): {100 * share:.2f} % of the op's kernel time", flush=True)
    return 0


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(*[int(x) for x in args[1:4]])
    no_profile = "--no-profile" in args
    a = [int(x) for x in args if x != "--no-profile"] or [32, 8, 4096, 16, 8, 2048]
    _hip.require_device()
    for i in range(0, len(a), 3):
        hq, hkv, S = a[i:i + 3]
        run = setup(hq, hkv, S)
        flop = 4.0 * S * S * D * hq / 2
        us16, us8 = time_us(run, "pgk_sdpa_causal"), time_us(run, "pgk_sdpa_causal_fp8")
        print(f"Hq={hq} Hkv={hkv} S={S} D={D}:  bf16 {us16:9.1f} us {flop / us16 / 1e6:7.1f} TFLOP/s   fp8 {us8:9.1f} us {flop / us8 / 1e6:7.1f} TFLOP/s"
              f"   fp8/bf16 speed ratio {us16 / us8:5.3f}", flush=True)
    if no_profile:
        return 0
    for i in range(0, len(a), 3):      # one profiled run per shape; stop at the first that fails
        if profile(*a[i:i + 3]):
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
