"""Time the integer ops beside their fp8 / NVF4 counterparts in one process.
usage: int8_bench.py [gemm] [decode] [switch]
  gemm:   gemm_int8_int32, matmul_int8_dequant (bf16 out), gemm_int4_int32 and gemm_fp8_fp8_blockwise_nt (unit scales) at 4096^3
          and 8192^3: same operand bytes as fp8 for int8, half for int4.
  decode: int4_gemv, linear_int8 (M = 1, bf16), gemv_nvf4_bf16 and gemv_fp8_bf16 at (K, N) = (4096, 14336) and (14336, 4096), as
          TB/s of weight bytes; every kind rotates over enough weight sets (>= 640 MB) that the timed weights are not in the L3.
  switch: linear_int8 at M = 1, 2, 4, 8 on both leaves (PGK_LIN8_STREAM_MAX_M = 8 / 0) at (K, N) = (4096, 14336), weights rotating as in decode: the row count
          at which int8_plan.h switches from the streaming kernel to the MFMA tile loop is set from these lines.
The variants of a row are timed in alternating device-event windows (A B C A B C ...) after 3 warm-up calls each; a figure is the
median of a variant's 6 windows, and `aa` is the median of its even windows over the median of its odd ones - the variant
against itself, the spread below which a difference between two variants means nothing."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from nvf4_bench import ROTATE_BYTES, fill  # noqa: E402
from pygpukit_amd import _hip, ops  # noqa: E402
from pygpukit_amd.core.array import GPUArray  # noqa: E402
from pygpukit_amd.core.dtypes import bfloat16, float32, int8, int32, uint8  # noqa: E402
from pygpukit_amd.ops.matmul.generic import gemm_plan  # noqa: E402

WINDOWS = 6


def alternate(variants: dict, n: int) -> dict:
    """name -> (median us per call, even-window median / odd-window median)."""
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        _hip.call("pgk_event_create", C.byref(e))
    for fn in variants.values():
        for _ in range(3):
            fn()
    us = {name: [] for name in variants}
    for _ in range(WINDOWS):
        for name, fn in variants.items():
            _hip.call("pgk_event_record", ev[0], None)
            for _ in range(n):
                fn()
            _hip.call("pgk_event_record", ev[1], None)
            _hip.call("pgk_event_sync", ev[1])
            t = C.c_float()
            _hip.call("pgk_event_elapsed_ms", ev[0], ev[1], C.byref(t))
            us[name].append(t.value / n * 1e3)
    for e in ev:
        _hip.call("pgk_event_destroy", e)
    return {name: (float(np.median(v)), float(np.median(v[0::2]) / np.median(v[1::2]))) for name, v in us.items()}


def bench_gemm():
    for S in (4096, 8192):
        M = N = K = S
        flop = 2.0 * M * N * K
        a8, w8, a4, w4 = GPUArray((M, K), int8), GPUArray((N, K), int8), GPUArray((M, K // 2), uint8), GPUArray((N, K // 2), uint8)
        f8a, f8w = GPUArray((M, K), uint8), GPUArray((N, K), uint8)
        for i, (arr, kind) in enumerate(((a8, "codes"), (w8, "codes"), (a4, "codes"), (w4, "codes"), (f8a, "fp8"), (f8w, "fp8"))):
            fill(arr, i, kind)
        d32, d16 = GPUArray((M, N), int32), GPUArray((M, N), bfloat16)
        sa, sw = GPUArray((M,), float32), GPUArray((N,), float32)
        sa.copy_from_numpy(np.full(M, 0.01, np.float32))
        sw.copy_from_numpy(np.full(N, 0.01, np.float32))
        fsa, fsw = GPUArray((M, K // 128), float32), GPUArray((N // 128, K // 128), bfloat16)
        fsa.copy_from_numpy(np.ones((M, K // 128), np.float32))
        fsw.copy_from_numpy(np.full((N // 128, K // 128), 0x3F80, np.uint16))
        res = alternate({
            "gemm_int8_int32": lambda: ops.gemm_int8_int32_sm120(a8, w8, d32),
            "matmul_int8_dequant": lambda: ops.matmul_int8_dequant(a8, sa, w8, sw, out=d16),
            "gemm_int4_int32": lambda: ops.gemm_int4_int32_sm120(a4, w4, d32),
            "gemm_fp8_fp8_blockwise_nt": lambda: ops.gemm_fp8_fp8_blockwise_nt(f8a, f8w, fsa, fsw, out=d16),
        }, 10 if S > 4096 else 50)
        for name, (us, aa) in res.items():
            print(f"gemm M=N=K={S}: {name:26s} {us:9.1f} us {flop / us / 1e6:7.1f} Top/s  aa {aa:.3f}  "
                  f"[{ops.int_gemm_plan('gemm_int4' if 'int4' in name else 'gemm_int8', M, N, K) if 'int' in name else gemm_plan('fp8_nt', M, N, K, 'bfloat16')}]",
                  flush=True)


def rotating_step(make, fills, set_bytes, run):
    sets = [make() for _ in range(max(2, -(-ROTATE_BYTES // set_bytes)))]
    for i, w in enumerate(sets):
        for j, (arr, kind) in enumerate(zip(w, fills)):
            fill(arr, 10 * i + j, kind)
    it = [0]

    def step():
        run(sets[it[0] % len(sets)])
        it[0] += 1
    return step, len(sets)


def bench_decode():
    for K, N in ((4096, 14336), (14336, 4096)):
        a16, a4 = GPUArray((K,), bfloat16), GPUArray((K // 2,), uint8)
        x16 = GPUArray((1, K), bfloat16)
        fill(a16, 1, "bf16")
        fill(x16, 1, "bf16")
        fill(a4, 2, "codes")
        o16, o32 = GPUArray((N,), bfloat16), GPUArray((N,), int32)
        s8 = GPUArray((N,), bfloat16)
        fill(s8, 3, "fp8_scale")
        kinds = {
            "int4_gemv": (K // 2 * N, lambda: (GPUArray((N, K // 2), uint8),), ("codes",), lambda w: ops.int4_gemv_int32_sm120(a4, w[0], o32, 0.5, 0.5)),
            "linear_int8": (K * N, lambda: (GPUArray((N, K), int8),), ("codes",), lambda w: ops.linear_int8(x16, w[0], s8)),
            "gemv_nvf4_bf16": (K // 2 * N + K // 32 * N, lambda: (GPUArray((K // 2, N), uint8), GPUArray((K // 32, N), uint8)), ("codes", "nvf4_scale"),
                               lambda w: ops.gemv_nvf4_bf16(a16, w[0], w[1], out=o16)),
            "gemv_fp8_bf16": (K * N + (N // 128) * (K // 128) * 2, lambda: (GPUArray((N, K), uint8), GPUArray((N // 128, K // 128), bfloat16)),
                              ("fp8", "fp8_scale"), lambda w: ops.gemv_fp8_bf16(a16, w[0], w[1], out=o16)),
        }
        steps, nsets = {}, 0
        for name, (wbytes, make, fills, run) in kinds.items():
            steps[name], n = rotating_step(make, fills, wbytes, run)
            nsets = max(nsets, n)
        res = alternate(steps, 8 * nsets)
        for name, (us, aa) in res.items():
            print(f"decode K={K} N={N}: {name:16s} {us:8.1f} us {kinds[name][0] / us / 1e6:5.2f} TB/s of {kinds[name][0] / 1e6:6.1f} MB weights  aa {aa:.3f}",
                  flush=True)
        del steps, kinds


def bench_switch():
    K, N = 4096, 14336
    ws, s = [GPUArray((N, K), int8) for _ in range(-(-ROTATE_BYTES // (N * K)))], GPUArray((N,), bfloat16)
    for i, w in enumerate(ws):
        fill(w, i, "codes")
    fill(s, 2, "fp8_scale")
    it = [0]
    for M in (1, 2, 4, 8):
        x = GPUArray((M, K), bfloat16)
        fill(x, 3, "bf16")

        def run(max_m):
            os.environ["PGK_LIN8_STREAM_MAX_M"] = str(max_m)
            ops.linear_int8(x, ws[it[0] % len(ws)], s)
            it[0] += 1
        os.environ["PGK_LIN8_STREAM_MAX_M"] = "8"
        leaf_s = ops.int_gemm_plan("linear_int8", M, N, K)
        os.environ["PGK_LIN8_STREAM_MAX_M"] = "0"
        leaf_m = ops.int_gemm_plan("linear_int8", M, N, K)
        res = alternate({leaf_s: lambda: run(8), leaf_m: lambda: run(0)}, 50)
        print(f"switch M={M} K={K} N={N}: " + "  ".join(f"{name} {us:7.1f} us aa {aa:.3f}" for name, (us, aa) in res.items()), flush=True)
    os.environ.pop("PGK_LIN8_STREAM_MAX_M", None)


def main():
    _hip.require_device()
    what = sys.argv[1:] or ["gemm", "decode", "switch"]
    if "gemm" in what:
        bench_gemm()
    if "decode" in what:
        bench_decode()
    if "switch" in what:
        bench_switch()


if __name__ == "__main__":
    main()
