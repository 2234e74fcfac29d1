"""Time MLA decode attention, sdpa_mla_fixed_cache, against the composition available without it, in one process with alternating
windows: per round every variant once, then every variant again (A'), N calls each between device events after a warm-up of all of
them.  bf16, H = 128 and 16, contexts 512, 4096, 32768 and 131072 (the cache as long as the context), q_len 1 and 4.

  (a) sdpa_mla_fixed_cache: one launch over the latent cache [ctx, 576] (plus the merge launch when the plan has several chunks);
  (b) matmul_nt -> softmax -> matmul on the same absorbed operands, the [q_len H, ctx] scores in global memory.  (b) is given every
      advantage: the scale is folded into q beforehand, the latent columns are a contiguous [ctx, 512] copy made beforehand, and at
      q_len 4 it applies NO causal mask (it computes something slightly different and cheaper).

Prints the median us per call of (a), the ratio a / b, the achieved bytes/s of latent rows (ctx x 1152 B) and FLOP/s
(2 x cols x ctx x (576 + 512)) of (a), the hardware minimum from the peaks below with which of the two bounds it, (a)'s share of it,
and the spread of each variant against itself (A' / A: the margin inside which two numbers are "the same").  Not a pass / fail gate.

--prefill times a prompt chunk instead: sdpa_mla_prefill with its kv_b_proj GEMM against the absorbed form (prefill() below).

--paged times a decode BATCH over a paged latent cache instead (paged() below): sdpa_mla_paged against sdpa_mla_fixed_cache per sequence.

usage: mla_bench.py [--prefill | --paged] [--rounds N] [--out FILE]"""
import argparse, ctypes as C, os, statistics, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from pygpukit_amd import _hip
from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import bfloat16
from pygpukit_amd.core.factory import from_numpy

PEAK_BYTES, PEAK_FLOPS = 8.0e12, 2.5e15          # MI355X: HBM bytes/s, dense bf16 MFMA FLOP/s
SCALE = 192 ** -0.5
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


def prefill(a, timer, rng):
    """--prefill: a prompt chunk S = T of 512, 2048 and 8192 rows, bf16, H = 128 and 16, nope = v = 128.
      (a) what MLAttention.forward_prefill runs between the cache write and o_proj: the kv_b_proj GEMM [T, 512] -> [T, H 256] and
          sdpa_mla_prefill;
      (b) what forward_fixed_cache runs for the same chunk: q_abs = q_nope . W_UK per head (batched_matmul between two
          transpose_3d_021), the pack of [q_abs | q_pe], sdpa_mla_fixed_cache with q_len = S, out . W_UV^T per head (the same).
    Share: of the matrix pipe's time for the textbook form's 4 S T / 2 (192 + 128) H flops, for both."""
    from pygpukit_amd.ops.matmul import batched_matmul, matmul_nt, transpose
    from pygpukit_amd.ops.nn import sdpa_mla_fixed_cache, sdpa_mla_prefill, sdpa_mla_prefill_plan
    from pygpukit_amd.ops.tensor import concat_axis0, transpose_3d_021
    say("| H | S = T | grid | (a) us | (b) us | a / b | matrix-pipe minimum us | share of it a, b | A'/A a, b |")
    say("|---|---|---|---|---|---|---|---|---|")
    for heads in (128, 16):
        w_kvb = bf16(rng.standard_normal((heads * 256, 512)) * 0.05)
        w_uk, w_uv_t = bf16(rng.standard_normal((heads, 128, 512)) * 0.05), bf16(rng.standard_normal((heads, 512, 128)) * 0.05)
        qn_block, qp_block = rng.standard_normal((64, heads, 128)), rng.standard_normal((64, heads, 64))
        for s in (512, 2048, 8192):
            cache = bf16(np.tile(rng.standard_normal((512, 576)), (s // 512, 1)))
            latent = bf16(np.tile(rng.standard_normal((512, 512)), (s // 512, 1)))
            q_nope, q_pe = bf16(np.tile(qn_block, (s // 64, 1, 1))), bf16(np.tile(qp_block, (s // 64, 1, 1)))
            out_a, out_b = GPUArray((s, heads, 128), bfloat16), GPUArray((s, heads, 512), bfloat16)

            def run_a():
                sdpa_mla_prefill(q_nope, q_pe, matmul_nt(latent, w_kvb).view((s, heads, 256)), cache, out_a, s, SCALE)

            def run_b():
                q_abs = transpose_3d_021(batched_matmul(transpose_3d_021(q_nope), w_uk)).view((s * heads, 512))
                q = transpose(concat_axis0(transpose(q_abs), transpose(q_pe.view((s * heads, 64))))).view((s, heads, 576))
                sdpa_mla_fixed_cache(q, cache, out_b, s, SCALE)
                return transpose_3d_021(batched_matmul(transpose_3d_021(out_b), w_uv_t))

            med, floor = measure(timer, {"a": run_a, "b": run_b}, a.rounds, 20 if s < 2048 else (5 if s < 8192 else 2))
            t_f = 4.0 * s * s / 2 * (192 + 128) * heads / PEAK_FLOPS * 1e6
            ratio, spread = med["a"] / med["b"], max(abs(floor["a"] - 1), abs(floor["b"] - 1))
            verdict = f"{ratio:.3f}" if ratio < 1 - spread else f"{ratio:.3f} (not faster)"
            say(f"| {heads} | {s} | {sdpa_mla_prefill_plan(heads, s, s, 'bfloat16')[1]} | {med['a']:.1f} | {med['b']:.1f} | {verdict} | {t_f:.1f} | "
                f"{t_f / med['a']:.3f}, {t_f / med['b']:.3f} | {floor['a']:.3f}, {floor['b']:.3f} |")


def paged(a, timer, rng):
    """--paged: 32 sequences, q_len 1, block_size 64, bf16, H = 128 and 16; every context 512 / 4096 / 32768, and one ragged batch with
    the contexts spread geometrically from 64 to 32768.  Pages are dealt out in a random order.
      (a) sdpa_mla_paged: one launch for the batch (plus the merge), the lengths on the device;
      (b) ONE gather launch of every sequence's pages into contiguous caches (an embedding lookup over the pages as rows of
          64 x 576, the cheapest gather the project has), then sdpa_mla_fixed_cache per sequence;
      (c) sdpa_mla_fixed_cache per sequence on contiguous caches that never were paged (no gather at all).
    a / b and a / c carry "(not faster)" unless below 1 by more than the larger A'/A spread of the pair.  GB/s: (a)'s latent rows,
    sum of contexts x 1152 B, and their share of the 8 TB/s peak.  Then the writer: mla_reshape_and_cache against mla_cache_write."""
    from pygpukit_amd.llm.layers.rope import precompute_freqs_cis
    from pygpukit_amd.ops.nn import (allocate_mla_cache, mla_cache_write, mla_reshape_and_cache, sdpa_mla_fixed_cache, sdpa_mla_paged,
                                     sdpa_mla_paged_plan)
    from pygpukit_amd.ops.paged import gather_embeddings
    nseq, bs, row_b = 32, 64, 1152
    block = bf16(rng.standard_normal((4096, 576)))                   # repeated: the time does not depend on the values
    i32 = lambda x: from_numpy(np.ascontiguousarray(x, np.int32))    # noqa: E731
    say("| H | contexts | grid (tiles, chunks, seqs) | (a) us | (b) us | (c) us | a / b | a / c | (a) latent rows GB/s | of 8 TB/s | A'/A a, b, c |")
    say("|---|---|---|---|---|---|---|---|---|---|---|")
    batches = [(str(c), [c] * nseq) for c in (512, 4096, 32768)] + [("64..32768 ragged", [int(round(64 * 512 ** (i / (nseq - 1)))) for i in range(nseq)])]
    for label, ctxs in batches:
        need = [-(-c // bs) for c in ctxs]
        nblk, bound = sum(need), max(ctxs)
        pages, perm = allocate_mla_cache(nblk, bs, bfloat16), rng.permutation(nblk).astype(np.int32)
        for k in range(0, nblk * bs, 4096):                          # fill the pages with the block
            n = min(4096, nblk * bs - k)
            _hip.call("pgk_memcpy_d2d", pages.data_ptr() + k * row_b, block.data_ptr(), n * row_b, None)
        first = np.concatenate([[0], np.cumsum(need)])
        tables = np.zeros((nseq, max(need)), np.int32)
        for b in range(nseq): tables[b, :need[b]] = perm[first[b]:first[b + 1]]
        tables_d, lens_d, ids = i32(tables), i32(ctxs), i32(perm)
        table2d = pages.view((nblk, bs * 576))
        flat = [GPUArray((need[b] * bs, 576), bfloat16) for b in range(nseq)]
        for b in range(nseq):
            for k in range(0, need[b] * bs, 4096):
                _hip.call("pgk_memcpy_d2d", flat[b].data_ptr() + k * row_b, block.data_ptr(), min(4096, need[b] * bs - k) * row_b, None)
        for heads in (128, 16):
            q = bf16(rng.standard_normal((nseq, 1, heads, 576)))
            out, qs, outs = GPUArray((nseq, 1, heads, 512), bfloat16), [], []
            for b in range(nseq):
                qs.append(q._view(b * heads * 576, (1, heads, 576))); outs.append(out._view(b * heads * 512, (1, heads, 512)))

            def run_b():
                g = gather_embeddings(ids, table2d, nblk)
                for b in range(nseq):
                    sdpa_mla_fixed_cache(qs[b], g._view(int(first[b]) * bs * 576, (need[b] * bs, 576)), outs[b], ctxs[b], SCALE)

            def run_c():
                for b in range(nseq): sdpa_mla_fixed_cache(qs[b], flat[b], outs[b], ctxs[b], SCALE)

            med, floor = measure(timer, {"a": lambda: sdpa_mla_paged(q, pages, tables_d, lens_d, out, bound, SCALE), "b": run_b, "c": run_c},
                                 a.rounds, 50 if bound < 32768 else 10)

            def verdict(k):
                ratio, spread = med["a"] / med[k], max(abs(floor["a"] - 1), abs(floor[k] - 1))
                return f"{ratio:.3f}" if ratio < 1 - spread else f"{ratio:.3f} (not faster)"

            rate = sum(ctxs) * row_b / med["a"] / 1e3
            say(f"| {heads} | {label} | {sdpa_mla_paged_plan(heads, 1, nseq, bound, 'bfloat16')[1]} | {med['a']:.1f} | {med['b']:.1f} | {med['c']:.1f} | "
                f"{verdict('b')} | {verdict('c')} | {rate:.0f} | {rate * 1e9 / PEAK_BYTES:.3f} | {floor['a']:.3f}, {floor['b']:.3f}, {floor['c']:.3f} |")
        del pages, flat
    say()
    say("| tokens | mla_reshape_and_cache us | mla_cache_write us | paged / contiguous | A'/A paged, contiguous |")
    say("|---|---|---|---|---|")
    cos, sin = (from_numpy(np.ascontiguousarray(t, np.float32)) for t in precompute_freqs_cis(64, 4096))
    gamma = bf16(1.0 + 0.1 * rng.standard_normal(512))
    pages, flat1 = allocate_mla_cache(64, bs, bfloat16), GPUArray((4096, 576), bfloat16)
    for n in (32, 4096):
        kv_a, pos, slots = block._view(0, (n, 576)), i32(rng.permutation(4096)[:n]), i32(rng.permutation(4096)[:n])
        med, floor = measure(timer, {"p": lambda: mla_reshape_and_cache(kv_a, gamma, cos, sin, pos, pages, slots),
                                     "c": lambda: mla_cache_write(kv_a, gamma, cos, sin, flat1, 0)}, a.rounds, 20)
        say(f"| {n} | {med['p']:.1f} | {med['c']:.1f} | {med['p'] / med['c']:.3f} | {floor['p']:.3f}, {floor['c']:.3f} |")


def decode(a, timer, rng):
    from pygpukit_amd.ops import matmul, matmul_nt, softmax
    from pygpukit_amd.ops.nn import sdpa_mla_fixed_cache, sdpa_mla_plan
    block = rng.standard_normal((512, 576)).astype(np.float32)       # repeated: the time does not depend on the values
    say("| H | q_len | context | plan (columns, chunks) | (a) us | a / b | latent rows GB/s | TFLOP/s | hardware minimum us (bound) | share of it | A'/A a, b |")
    say("|---|---|---|---|---|---|---|---|---|---|---|")
    for ctx in (512, 4096, 32768, 131072):
        rows = np.tile(block, (ctx // 512, 1))
        cache, latent = bf16(rows), bf16(rows[:, :512])
        for heads in (128, 16):
            for q_len in (1, 4):
                cols = heads * q_len
                qh = rng.standard_normal((q_len, heads, 576)).astype(np.float32)
                q, q_scaled, out = bf16(qh), bf16(qh.reshape(cols, 576) * SCALE), GPUArray((q_len, heads, 512), bfloat16)
                med, floor = measure(timer, {"a": lambda: sdpa_mla_fixed_cache(q, cache, out, ctx, SCALE),
                                             "b": lambda: matmul(softmax(matmul_nt(q_scaled, cache)), latent)}, a.rounds, 20 if ctx < 32768 else 5)
                nbytes, flops = ctx * 1152, 2.0 * cols * ctx * (576 + 512)
                t_b, t_f = nbytes / PEAK_BYTES * 1e6, flops / PEAK_FLOPS * 1e6
                ratio = med["a"] / med["b"]
                spread = max(abs(floor["a"] - 1), abs(floor["b"] - 1))
                verdict = f"{ratio:.3f}" if ratio < 1 - spread else f"{ratio:.3f} (not faster)"
                say(f"| {heads} | {q_len} | {ctx} | {sdpa_mla_plan(heads, q_len, ctx, 'bfloat16')[1:]} | {med['a']:.1f} | {verdict} | "
                    f"{nbytes / med['a'] / 1e3:.0f} | {flops / med['a'] / 1e6:.1f} | {max(t_b, t_f):.2f} ({'bytes' if t_b >= t_f else 'matrix'}) | "
                    f"{max(t_b, t_f) / med['a']:.3f} | {floor['a']:.3f}, {floor['b']:.3f} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--prefill", action="store_true", help="time sdpa_mla_prefill against the absorbed form on a prompt chunk instead")
    ap.add_argument("--paged", action="store_true", help="time sdpa_mla_paged on a decode batch against sdpa_mla_fixed_cache per sequence instead")
    a = ap.parse_args()
    (prefill if a.prefill else paged if a.paged else decode)(a, Timer(), np.random.default_rng(0))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
