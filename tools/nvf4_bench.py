"""Time the NVF4 ops beside their bf16 / fp8 counterparts in one run.
usage: nvf4_bench.py [gemv] [gemm]
  GEMV at (K,N) = (1024,151936), (4096,14336), (14336,4096), (4096,128256): gemv_nvf4_bf16 on [K/2,N] data + [K/32,N]
       scales, gemv_bf16 on [N,K] bf16 and gemv_fp8_bf16 on [N,K] e4m3 + [N/128,K/128] scales.  Each kind rotates
       over enough weight sets (>= 640 MB together) that the timed weights are not resident in the 256 MiB L3.
       TB/s = (weight + scale + a + out bytes) / time.
  GEMM at the prefill shapes of profiles/r04_fp8nn_gemm_bench.log: matmul_nvf4_bf16_sm120 end to end (both
       quantise-and-pack kernels + the FP4 MFMA kernel), pgk_gemm_fp4_nt alone on packed operands, and the fp8 NT
       kernel (pgk_gemm_fp8_nt, unit scales) on the same shape.
Each figure: median of 5 device-event windows of n calls, after 3 warm-up calls."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pygpukit_amd import _hip  # noqa: E402
from pygpukit_amd.core.array import GPUArray  # noqa: E402
from pygpukit_amd.core.dtypes import bfloat16, float32, uint8  # noqa: E402
from pygpukit_amd.ops import gemv_bf16, gemv_fp8_bf16, gemv_nvf4_bf16, matmul_nvf4_bf16_sm120  # noqa: E402

GEMV_SHAPES = [(1024, 151936), (4096, 14336), (14336, 4096), (4096, 128256)]
GEMM_SHAPES = [(4096, 4096, 4096), (8192, 8192, 8192), (4096, 6144, 4096), (4096, 28672, 4096), (4096, 4096, 14336)]
ROTATE_BYTES = 640 << 20


def fill(arr: GPUArray, seed: int, kind: str) -> None:
    """A 16 MiB random block repeated over the array (device copies)."""
    rng = np.random.default_rng(seed)
    n = min(arr.nbytes, 16 << 20)
    if kind == "bf16":
        blk = ((rng.standard_normal(n // 2).astype(np.float32) * 0.5).view(np.uint32) >> 16).astype(np.uint16).view(np.uint8)
    elif kind == "fp8":     # e4m3 codes with exponent fields 5..9 (no NaN codes)
        blk = (rng.integers(0, 2, n) << 7 | rng.integers(5, 10, n) << 3 | rng.integers(0, 8, n)).astype(np.uint8)
    elif kind == "nvf4_scale":
        blk = rng.integers(0x28, 0x40, n).astype(np.uint8)
    elif kind == "fp8_scale":   # bf16 powers of two around 2^-8
        blk = (np.exp2(rng.integers(-10, -6, n // 2)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16).view(np.uint8)
    else:
        blk = rng.integers(0, 256, n).astype(np.uint8)
    _hip.call("pgk_memcpy_h2d", arr._p, blk.ctypes.data_as(C.c_void_p), n, None)
    off = n
    while off < arr.nbytes:
        m = min(off, arr.nbytes - off)
        _hip.call("pgk_memcpy_d2d", C.c_void_p(arr.device_ptr + off), arr._p, m, None)
        off += m


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


def rotating(make, set_bytes):
    """Enough weight sets that one pass over them exceeds ROTATE_BYTES; returns (sets, call counter)."""
    nsets = max(2, -(-ROTATE_BYTES // set_bytes))
    return [make(i) for i in range(nsets)]


def bench_gemv():
    for K, N in GEMV_SHAPES:
        a = GPUArray((K,), bfloat16)
        fill(a, 1, "bf16")
        out = GPUArray((N,), bfloat16)
        io = 2 * K + 2 * N
        line = f"gemv K={K:5d} N={N:6d}:"
        kinds = [
            ("nvf4", K // 2 * N + (K + 31) // 32 * N,
             lambda i: (GPUArray((K // 2, N), uint8), GPUArray(((K + 31) // 32, N), uint8)),
             lambda w: gemv_nvf4_bf16(a, w[0], w[1], out=out), ("codes", "nvf4_scale")),
            ("fp8", K * N + (N // 128) * (K // 128) * 2,
             lambda i: (GPUArray((N, K), uint8), GPUArray((N // 128, K // 128), bfloat16)),
             lambda w: gemv_fp8_bf16(a, w[0], w[1], out=out), ("fp8", "fp8_scale")),
            ("bf16", 2 * K * N, lambda i: (GPUArray((N, K), bfloat16),), lambda w: gemv_bf16(a, w[0], out=out), ("bf16",)),
        ]
        for name, wbytes, make, run, fills in kinds:
            sets = rotating(make, wbytes)
            for i, w in enumerate(sets):
                for j, (arr, kind) in enumerate(zip(w, fills)):
                    fill(arr, 10 * i + j, kind)
            it = [0]

            def step():
                run(sets[it[0] % len(sets)])
                it[0] += 1
            us = timed(step, 4 * len(sets))
            line += f"  {name} {us:8.1f} us {(wbytes + io) / us / 1e6:5.2f} TB/s ({wbytes / 1e6:6.1f} MB x{len(sets)})"
            del sets
        print(line, flush=True)


def bench_gemm():
    for M, N, K in GEMM_SHAPES:
        flop = 2.0 * M * N * K
        a, b, d = GPUArray((M, K), bfloat16), GPUArray((K, N), bfloat16), GPUArray((M, N), bfloat16)
        fill(a, 1, "bf16")
        fill(b, 2, "bf16")
        n = 5 if flop > 2e12 else 20
        t_e2e = timed(lambda: matmul_nvf4_bf16_sm120(a, b, out=d), n)
        kp = (K + 127) // 128 * 128
        ws = GPUArray((int(_hip.load().pgk_gemm_nvf4_workspace_bytes(M, N, K)),), uint8)
        bp = C.c_void_p(ws.device_ptr + M * kp // 2)
        _hip.call("pgk_quantize_e2m1_unit", a._p, ws._p, M, K, 0, None)
        _hip.call("pgk_quantize_e2m1_unit", b._p, bp, N, K, 1, None)
        t_fp4 = timed(lambda: _hip.call("pgk_gemm_fp4_nt", ws._p, bp, d._p, M, N, kp, None), n)
        a8, w8 = GPUArray((M, K), uint8), GPUArray((N, K), uint8)
        fill(a8, 3, "fp8")
        fill(w8, 4, "fp8")
        sa, sw = GPUArray((M, K // 128), float32), GPUArray(((N + 127) // 128, K // 128), bfloat16)
        sa.copy_from_numpy(np.ones((M, K // 128), np.float32))
        sw.copy_from_numpy(np.full(((N + 127) // 128, K // 128), 0x3F80, np.uint16))
        t_fp8 = timed(lambda: _hip.call("pgk_gemm_fp8_nt", a8._p, sa._p, w8._p, sw._p, d._p, M, N, K, None), n)
        print(f"gemm M={M} N={N} K={K}:  nvf4 end-to-end {t_e2e:8.1f} us {flop / t_e2e / 1e6:7.1f} TFLOP/s  "
              f"fp4 kernel {t_fp4:8.1f} us {flop / t_fp4 / 1e6:7.1f} TFLOP/s  "
              f"fp8 NT kernel {t_fp8:8.1f} us {flop / t_fp8 / 1e6:7.1f} TFLOP/s", flush=True)
        del a, b, d, ws, a8, w8, sa, sw


def main():
    _hip.require_device()
    what = sys.argv[1:] or ["gemv", "gemm"]
    if "gemv" in what:
        bench_gemv()
    if "gemm" in what:
        bench_gemm()


if __name__ == "__main__":
    main()
