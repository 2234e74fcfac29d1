"""Time packed prefill attention over the paged KV cache against what serves the same tokens without it, in one process with
alternating windows: per round every variant once, then the first variant again (A'), N calls each between device events after a
warm-up of all of them.  Prints the median us per batch, the ratios, and the spread of the first variant against itself (A' / A:
the margin inside which two numbers are "the same").  Not a pass / fail gate.  bf16, Hq 32, Hkv 8, D 128, block_size 16, pages
dealt to the sequences in random order.

  (a) paged_attention_prefill: one launch for the whole batch, K / V read straight from the pages;
  (b) today's route: gather each sequence's pages into contiguous [Hkv, ctx, D] K and V (gather_embeddings over the cache as a
      table of rows; the row ids are built once, outside the timing), then sdpa_causal per sequence;
  (c) sdpa_causal per sequence on K / V that are contiguous already: the floor with no paging at all.

Batches: 8 x 512, 4 x 2048 and 1 x 8192 whole prompts, and a mixed step of 3 x 1024-token prompts plus 32 decode rows at context 2048.

usage: paged_prefill_bench.py [--rounds N] [--out FILE]"""
import argparse, os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from attn_window_bench import LINES, Timer, measure, say
from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import bfloat16
from pygpukit_amd.core.factory import from_numpy

HQ, HKV, D, BS = 32, 8, 128, 16
BATCHES = [("8 x 512", [(512, 512)] * 8, 10), ("4 x 2048", [(2048, 2048)] * 4, 5), ("1 x 8192", [(8192, 8192)], 3),
           ("3 x 1024 + 32 decode rows at 2048", [(1024, 1024)] * 3 + [(1, 2048)] * 32, 5)]


def dev(x):
    return from_numpy(np.ascontiguousarray(x, np.float32)).astype(bfloat16)


def bench(timer, name, pairs, n, rounds):
    from pygpukit_amd.ops.nn import sdpa_causal
    from pygpukit_amd.ops.paged import gather_embeddings, paged_attention_prefill, paged_prefill_plan
    rng = np.random.default_rng(len(pairs))
    need = [-(-ctx // BS) for _, ctx in pairs]
    pages = rng.permutation(sum(need)).astype(np.int32)
    tables = np.zeros((len(pairs), max(need)), np.int32)
    kc, vc = (np.zeros((sum(need), HKV, BS, D), np.float32) for _ in range(2))
    seqs, at = [], 0
    for b, (q_len, ctx) in enumerate(pairs):
        tables[b, :need[b]] = pages[at:at + need[b]]; at += need[b]
        pos = np.arange(ctx)
        page, off = tables[b][pos // BS], pos % BS
        k, v = D ** -0.25 * rng.standard_normal((HKV, ctx, D), dtype=np.float32), rng.standard_normal((HKV, ctx, D), dtype=np.float32)
        kc[page, :, off], vc[page, :, off] = k.transpose(1, 0, 2), v.transpose(1, 0, 2)
        q = D ** -0.25 * rng.standard_normal((HQ, q_len, D), dtype=np.float32)
        ids = ((page[None, :] * HKV + np.arange(HKV)[:, None]) * BS + off[None, :]).astype(np.int32).ravel()
        seqs.append(dict(q=q, qd=dev(q), k=dev(k), v=dev(v), ids=from_numpy(ids), ctx=ctx, out=GPUArray((HQ, q_len, D), bfloat16)))
    cu = np.concatenate([[0], np.cumsum([p[0] for p in pairs])]).astype(np.int32)
    qp, outp = dev(np.concatenate([s["q"].transpose(1, 0, 2) for s in seqs])), GPUArray((int(cu[-1]), HQ, D), bfloat16)
    kcd, vcd, tab, ctxs, cud = dev(kc), dev(vc), from_numpy(tables), from_numpy(np.array([p[1] for p in pairs], np.int32)), from_numpy(cu)
    k2, v2 = kcd.view((kcd.size // D, D)), vcd.view((vcd.size // D, D))
    mq = max(p[0] for p in pairs)

    def paged():
        paged_attention_prefill(qp, kcd, vcd, tab, ctxs, cud, out=outp, max_query_len=mq)

    def gathered():
        for s in seqs:
            k = gather_embeddings(s["ids"], k2, HKV * s["ctx"]).view((HKV, s["ctx"], D))
            v = gather_embeddings(s["ids"], v2, HKV * s["ctx"]).view((HKV, s["ctx"], D))
            sdpa_causal(s["qd"], k, v, out=s["out"])

    def contiguous():
        for s in seqs:
            sdpa_causal(s["qd"], s["k"], s["v"], out=s["out"])

    med, floor, lo, hi = measure(timer, {"a": paged, "b": gathered, "c": contiguous}, rounds, n)
    flops = 4.0 * HQ * D * sum(q_len * (ctx - q_len) + q_len * (q_len + 1) / 2 for q_len, ctx in pairs)
    say(f"{name}: plan {paged_prefill_plan(len(pairs), mq, HQ, HKV, D, 'bfloat16')}; (a) paged_attention_prefill {med['a']:.0f} us "
        f"({flops / med['a'] / 1e6:.0f} TFLOP/s of live work), (b) gather + sdpa_causal per sequence {med['b']:.0f} us, (c) sdpa_causal per "
        f"sequence on contiguous K / V {med['c']:.0f} us: a/b {med['a'] / med['b']:.3f}, a/c {med['a'] / med['c']:.3f}; A'/A {floor:.3f}, "
        f"windows {lo:.0f}..{hi:.0f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    timer = Timer()
    say(f"paged prefill, bfloat16, Hq {HQ} Hkv {HKV} D {D} block_size {BS}; median of {a.rounds} rounds")
    for name, pairs, n in BATCHES:
        bench(timer, name, pairs, n, a.rounds)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
