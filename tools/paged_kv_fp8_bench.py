"""Time the FP8 (e4m3) paged KV cache ops against the bf16 paged ops in one process with alternating windows: per round every
variant once, then every variant again (A'), N calls each between device events after a warm-up of all of them.  Prints the median
us per call, the time ratio next to the byte ratio, and the spread of each op against itself (A' / A: the margin inside which two
numbers are "the same").  Not a pass / fail gate.  bf16 queries, Hq 32, Hkv 8, D 128, block_size 16, pages dealt in random order;
the bf16 pages hold the dequantised codes, so both ops compute on the same values.

  (a) decode: paged_attention_v1_fp8 against paged_attention_v1, 32 sequences at contexts 512, 4096 and 32768 (byte ratio 0.5);
  (b) prefill: paged_attention_prefill_fp8 against paged_attention_prefill on the four batches of tools/paged_prefill_bench.py
      (byte ratio 0.5; 4 x 2048 and 1 x 8192 are bound by the MFMAs, not by bytes);
  (c) the writer: reshape_and_cache_fp8 against reshape_and_cache, 32 and 4096 tokens (2 x 2 bytes read, 2 x 1 written: 0.75).

usage: paged_kv_fp8_bench.py [--rounds N] [--out FILE] [--sections abc]"""
import argparse, os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from attn_kv_fp8_bench import LINES, Timer, measure, say
from oracle.cpu_ref import fp8_e4m3_table
from paged_prefill_bench import BATCHES
from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import bfloat16
from pygpukit_amd.core.factory import from_numpy, zeros

HQ, HKV, D, BS, SCALE = 32, 8, 128, 16, 0.25


def bf16(a):
    return from_numpy(np.ascontiguousarray(a, np.float32)).astype(bfloat16)


def pool(rng, ctxs):
    """-> code caches of magnitude 0.25 .. 3.75 with random signs (device, uint8), their dequantised bf16 twins, tables, lengths.
    A block of 2048 random pages repeated: the time does not depend on the values."""
    need = [-(-c // BS) for c in ctxs]
    pages = rng.permutation(sum(need)).astype(np.int32)
    tables, at = np.zeros((len(ctxs), max(need)), np.int32), 0
    for b, n in enumerate(need):
        tables[b, :n] = pages[at:at + n]; at += n
    block, shape = (min(sum(need), 2048), HKV, BS, D), (sum(need), HKV, BS, D)
    c8, c16 = [], []
    for _ in range(2):
        codes = rng.integers(0x28, 0x48, block, dtype=np.uint8) | (rng.integers(0, 2, block, dtype=np.uint8) << 7)
        words = ((fp8_e4m3_table()[codes] * SCALE).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)     # exact in bf16
        reps = (-(-shape[0] // block[0]), 1, 1, 1)
        c8.append(from_numpy(np.ascontiguousarray(np.tile(codes, reps)[:shape[0]])))
        c16.append(GPUArray(shape, bfloat16))
        c16[-1].copy_from_numpy(np.tile(words, reps)[:shape[0]])
    return c8, c16, from_numpy(tables), from_numpy(np.array(ctxs, np.int32))


def line(tag, what, names, med, floor, byte_ratio):
    ratio = med["fp8"] / med["bf16"]
    say(f"({tag}) {what}: {names[0]} {med['fp8']:.1f} us, {names[1]} {med['bf16']:.1f} us: fp8 / bf16 time ratio {ratio:.3f} against the byte "
        f"ratio {byte_ratio}; A'/A fp8 {floor['fp8']:.3f}, bf16 {floor['bf16']:.3f}")
    return ratio


def section_a(timer, rounds):
    from pygpukit_amd.ops.paged import paged_attention_v1, paged_attention_v1_fp8, paged_kv_fp8_plan
    rng = np.random.default_rng(0)
    sc = from_numpy(np.full(HKV, SCALE, np.float32))
    for ctx in (512, 4096, 32768):
        (k8, v8), (k16, v16), tab, ctxs = pool(rng, [ctx] * 32)
        q, out = bf16(rng.standard_normal((32, HQ, D)) * D ** -0.25), GPUArray((32, HQ, D), bfloat16)
        med, floor = measure(timer, {"fp8": lambda: paged_attention_v1_fp8(q, k8, v8, sc, sc, tab, ctxs, out=out, max_context=ctx),
                                     "bf16": lambda: paged_attention_v1(q, k16, v16, tab, ctxs, out=out, max_context=ctx)}, rounds, 20)
        rows = 2 * 32 * HKV * ctx * D
        line("a", f"decode 32 sequences at context {ctx}, plan {paged_kv_fp8_plan('decode', 32, ctx, HQ, HKV, D, 'bfloat16')}, "
             f"{rows / med['fp8'] / 1e3:.0f} GB/s of codes against {2 * rows / med['bf16'] / 1e3:.0f} GB/s of bf16 rows",
             ("paged_attention_v1_fp8", "paged_attention_v1"), med, floor, 0.5)


def section_b(timer, rounds):
    from pygpukit_amd.ops.paged import paged_attention_prefill, paged_attention_prefill_fp8
    sc = from_numpy(np.full(HKV, SCALE, np.float32))
    for name, pairs, n in BATCHES:
        rng = np.random.default_rng(len(pairs))
        (k8, v8), (k16, v16), tab, ctxs = pool(rng, [p[1] for p in pairs])
        cu = np.concatenate([[0], np.cumsum([p[0] for p in pairs])]).astype(np.int32)
        q, out = bf16(rng.standard_normal((int(cu[-1]), HQ, D)) * D ** -0.25), GPUArray((int(cu[-1]), HQ, D), bfloat16)
        cud, mq = from_numpy(cu), max(p[0] for p in pairs)
        med, floor = measure(timer, {"fp8": lambda: paged_attention_prefill_fp8(q, k8, v8, sc, sc, tab, ctxs, cud, out=out, max_query_len=mq),
                                     "bf16": lambda: paged_attention_prefill(q, k16, v16, tab, ctxs, cud, out=out, max_query_len=mq)}, rounds, n)
        ratio = line("b", f"prefill {name}", ("paged_attention_prefill_fp8", "paged_attention_prefill"), med, floor, 0.5)
        if name in ("4 x 2048", "1 x 8192"):        # compute-bound: the fp8 staging must cost no more than bf16's own spread
            spread = abs(floor["bf16"] - 1.0)
            say(f"    compute-bound row: fp8 is {'NOT ' if ratio > 1.0 + spread else ''}within the bf16 kernel's own spread "
                f"(ratio {ratio:.3f} against 1 + {spread:.3f})")


def section_c(timer, rounds):
    from pygpukit_amd.ops.paged import reshape_and_cache, reshape_and_cache_fp8
    rng = np.random.default_rng(2)
    blocks = 4096 // BS
    c8, c16 = [from_numpy(np.zeros((blocks, HKV, BS, D), np.uint8)) for _ in range(2)], [zeros((blocks, HKV, BS, D), bfloat16) for _ in range(2)]
    sc = from_numpy(np.full(HKV, 0.37, np.float32))
    for tokens in (32, 4096):
        k, v = bf16(rng.standard_normal((tokens, HKV, D))), bf16(rng.standard_normal((tokens, HKV, D)))
        slots = from_numpy(rng.permutation(4096)[:tokens].astype(np.int32))
        med, floor = measure(timer, {"fp8": lambda: reshape_and_cache_fp8(k, v, c8[0], c8[1], slots, sc, sc),
                                     "bf16": lambda: reshape_and_cache(k, v, c16[0], c16[1], slots)}, rounds, 20)
        line("c", f"writer {tokens} tokens", ("reshape_and_cache_fp8", "reshape_and_cache"), med, floor, 0.75)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sections", default="abc")
    a = ap.parse_args()
    timer = Timer()
    for s, fn in (("a", section_a), ("b", section_b), ("c", section_c)):
        if s in a.sections:
            fn(timer, a.rounds)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
