"""Staircase inputs for exact causal-mask checks of the attention kernels (NumPy only).

A whole-tensor relative error on random data does not see a mask that is off by one key at a tile edge (the contrast case
of tests/test_attention_mask_cpu.py records the figures).  Here Q and K are built so that the score of (query i, key j)
grows steeply and exactly with j, the same for every query:

    K[:, j, c] = (height(j) >> 3c) & 7        c = 0 .. nd-1    the height of a key (its position, unless said otherwise) in base 8
    Q[:, :, c] = s * 8**c                     s a power of two -> q . k = s * height(j) + noise
    every other column: N(0, 1) in K, N(0, 1) / 8 in Q, so that all k-steps of the kernels carry data
    V = N(0, 1), different in every kv head

Digits 0..7 and powers of two are exact in bf16, f16 and (under the per-head power-of-two scale of the fp8 quantiser) e4m3.
Neighbouring keys are `s * op_scale` >= 60 natural-log units apart (op_scale: what the op multiplies the scores by), so the
softmax weight of every key but the highest visible one is below 2**-80 and each output row IS the V row of its last visible
key: out[h, i] == V[h // rep, mask_off + i].  One more visible key returns the next V row, one fewer (a dropped tile, an
empty split) the previous one, a zero or a NaN; a wrong kv head, page or cache row returns some other V row.

Every builder's precondition is checked on the CPU (check_precondition): the op's own fp64 oracle on the rounded inputs
must return the expected V rows within 2**-20 in every element.
"""

from __future__ import annotations

import functools
import math

import numpy as np

from oracle import cpu_ref as O

F32 = np.float32
PRECONDITION = 2.0 ** -20
MIN_STEP = 60.0                  # natural-log units between neighbouring keys after the op's own scaling
F16_MAX = 65504.0


# ---- number formats ----------------------------------------------------------------------------------------------------

def round_to(x, dtype: str) -> np.ndarray:
    """Values -> the nearest value of `dtype` ("f32", "f16", "bf16"; ties to even), as float32."""
    x = np.ascontiguousarray(x, F32)
    if dtype == "f32":
        return x
    if dtype == "f16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16).astype(F32)
    assert dtype == "bf16", dtype
    return O.bf16_bits_to_f32(O.f32_to_bf16_bits(x))


def to_words(x, dtype: str) -> np.ndarray:
    """float32 values of `dtype` -> what the device holds: uint16 words for bf16 / f16, the float32 array itself for f32."""
    x = np.ascontiguousarray(x, F32)
    if dtype == "f32":
        return x
    return O.f32_to_bf16_bits(x) if dtype == "bf16" else x.astype(np.float16).view(np.uint16)


def from_words(w, dtype: str) -> np.ndarray:
    if dtype == "f32":
        return np.asarray(w, F32)
    w = np.ascontiguousarray(w, np.uint16)
    return O.bf16_bits_to_f32(w) if dtype == "bf16" else w.view(np.float16).astype(F32)


# ---- the construction ---------------------------------------------------------------------------------------------------

def digits_for(n_heights: int) -> int:
    """Base-8 digits that hold the heights 0 .. n_heights - 1."""
    nd = 1
    while 8 ** nd < n_heights:
        nd += 1
    return nd


def stair_s(op_scale: float) -> int:
    """Smallest power of two s with s * op_scale >= MIN_STEP."""
    s = 1
    while s * op_scale < MIN_STEP:
        s *= 2
    return s


def n_digits(n_heights: int, dtype: str) -> int:
    """Four digits (heights below 4096) wherever the format holds s * 8**3; f16 tops out at 65504, so f16 inputs carry only
    the digits their heights need."""
    nd = digits_for(n_heights)
    assert nd <= 4, f"{n_heights} heights need more than four base-8 digits"
    return nd if dtype == "f16" else 4


def stair_k(rng, heads: int, heights, d: int, nd: int, dtype: str) -> np.ndarray:
    """K [heads, len(heights), d]: row j carries heights[j] in base 8 in columns 0 .. nd-1, noise elsewhere."""
    heights = np.asarray(heights, np.int64)
    assert heights.min() >= 0 and heights.max() < 8 ** nd and nd <= d
    k = round_to(rng.standard_normal((heads, heights.size, d)), dtype)
    for c in range(nd):
        k[:, :, c] = ((heights >> (3 * c)) & 7).astype(F32)
    return k


def stair_q(rng, heads: int, rows: int, d: int, nd: int, s: int, dtype: str) -> np.ndarray:
    """Q [heads, rows, d]: the weights s * 8**c in columns 0 .. nd-1 (the same for every row), noise / 8 elsewhere."""
    assert s & (s - 1) == 0, "s must be a power of two"
    q = round_to(rng.standard_normal((heads, rows, d)) / 8.0, dtype)
    for c in range(nd):
        q[:, :, c] = F32(s * 8 ** c)
    assert np.array_equal(round_to(q, dtype), q) and np.isfinite(q).all(), "a weight is not finite in the storage type"
    if dtype == "f16":
        assert s * 8 ** (nd - 1) <= F16_MAX
    return q


def stair_v(rng, heads: int, rows: int, d: int, dtype: str) -> np.ndarray:
    return round_to(rng.standard_normal((heads, rows, d)), dtype)


class Stair:
    """One dense case: q [hq, q_len, d], k / v [hkv, kv_len, d] as float32 values of `dtype`, read-only."""

    def __init__(self, hq, hkv, q_len, kv_len, d, dtype, s, seed):
        rng = np.random.default_rng(seed)
        self.shape = (hq, hkv, q_len, kv_len, d)
        self.dtype, self.s, self.rep = dtype, s, hq // hkv
        self.nd = n_digits(kv_len, dtype)
        self.q = stair_q(rng, hq, q_len, d, self.nd, s, dtype)
        self.k = stair_k(rng, hkv, np.arange(kv_len), d, self.nd, dtype)
        self.v = stair_v(rng, hkv, kv_len, d, dtype)
        for a in (self.q, self.k, self.v):
            a.setflags(write=False)

    def expected(self, mask_off: int, q_len: int | None = None) -> np.ndarray:
        """[hq, q_len, d]: row i of head h is V[h // rep, mask_off + i]."""
        hq, _, ql, kv_len, _ = self.shape
        q_len = ql if q_len is None else q_len
        rows = mask_off + np.arange(q_len)
        assert rows.min() >= 0 and rows.max() < kv_len
        return self.v[np.arange(hq) // self.rep][:, rows]

    def f64(self):
        return tuple(np.asarray(a, np.float64) for a in (self.q, self.k, self.v))


@functools.lru_cache(maxsize=None)
def make_stair(hq, hkv, q_len, kv_len, d, dtype="bf16", op_scale=1.0) -> Stair:
    """op_scale: what the op multiplies q . k by - 1.0 for the ops that take `scale` (the tests pass scale=1.0),
    irope_scale(d) for sdpa_irope."""
    s = stair_s(op_scale)
    assert s * op_scale >= MIN_STEP
    return Stair(hq, hkv, q_len, kv_len, d, dtype, s, seed=(hq * 7919 + hkv * 104729 + q_len * 31 + kv_len) * 131 + d + len(dtype))


def irope_scale(d: int) -> float:
    """sdpa_irope has no scale argument and divides by sqrt(d); its temperature is >= 1 and only widens the step."""
    return 1.0 / math.sqrt(d)


class PagedStair:
    """paged_attention_v1 inputs: q [num_seqs, hq, d], caches [num_blocks, hkv, block_size, d], tables, context lengths.
    The pages of a sequence are scattered by a permutation that never hands out page 0; page 0, every unreferenced page
    and the tail slots of each last page hold stairs higher than any valid key (and V rows of their own), and unused
    table entries point at page 0.  expected[s, h] = the V row written at slot ctx_s - 1 of sequence s."""

    def __init__(self, num_seqs, hq, hkv, d, bs, ctxs, dtype, s=64):
        ctxs = tuple(int(c) for c in ctxs)
        assert len(ctxs) == num_seqs
        rng = np.random.default_rng(sum((i + 3) * c for i, c in enumerate(ctxs)) * 977 + hq * 31 + d + bs + len(dtype))
        max_ctx = max(ctxs)
        nd = n_digits(2 * max_ctx, dtype)               # room for poison heights above every valid key
        npages = [(c + bs - 1) // bs for c in ctxs]
        max_blocks = max(npages) + 1                    # at least one unused table entry per sequence
        num_blocks = sum(npages) + 4
        perm = 1 + rng.permutation(num_blocks - 1)      # physical pages 1 .. num_blocks-1, scattered
        self.tables = np.zeros((num_seqs, max_blocks), np.int32)
        # every slot starts as poison: heights in [max_ctx, 8**nd)
        poison = rng.integers(max_ctx, 8 ** nd, num_blocks * bs)
        self.k = stair_k(rng, hkv, poison, d, nd, dtype).reshape(hkv, num_blocks, bs, d).transpose(1, 0, 2, 3).copy()
        self.v = stair_v(rng, hkv, num_blocks * bs, d, dtype).reshape(hkv, num_blocks, bs, d).transpose(1, 0, 2, 3).copy()
        self.q = np.empty((num_seqs, hq, d), F32)
        self.expected = np.empty((num_seqs, hq, d), F32)
        rep, nxt = hq // hkv, 0
        for i, ctx in enumerate(ctxs):
            self.q[i] = stair_q(rng, hq, 1, d, nd, s, dtype)[:, 0]
            ks = stair_k(rng, hkv, np.arange(ctx), d, nd, dtype)
            vs = stair_v(rng, hkv, ctx, d, dtype)
            for b in range(npages[i]):
                page = int(perm[nxt])
                nxt += 1
                self.tables[i, b] = page
                n = min(bs, ctx - b * bs)
                self.k[page, :, :n] = ks[:, b * bs:b * bs + n]
                self.v[page, :, :n] = vs[:, b * bs:b * bs + n]
            self.expected[i] = vs[np.arange(hq) // rep, ctx - 1]
        self.ctxs = np.array(ctxs, np.int32)
        self.dtype, self.max_ctx, self.nd = dtype, max_ctx, nd
        for a in (self.q, self.k, self.v, self.tables, self.ctxs, self.expected):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def make_paged(num_seqs, hq, hkv, d, bs, ctxs: tuple, dtype="bf16") -> PagedStair:
    return PagedStair(num_seqs, hq, hkv, d, bs, ctxs, dtype)


# ---- reference with a free mask (for mutated masks; the ops' own oracles have theirs built in) -------------------------

def attention_last(q, k, v, last, scale: float, *, row_scale=None, slopes=None, origin: int = 0) -> np.ndarray:
    """fp64 attention in which query row i sees the keys j <= last[i] (clipped to the keys there are; a row that sees none
    is zero): softmax_j(q_i . k_j * scale * row_scale[i] - slopes[h] * (origin + i - j)) . v, GQA by h // rep."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    hq, q_len, d = q.shape
    hkv, kv_len, _ = k.shape
    rep = hq // hkv
    last = np.minimum(np.asarray(last, np.int64), kv_len - 1)
    i, j = np.arange(q_len)[:, None], np.arange(kv_len)[None, :]
    seen = j <= last[:, None]
    rs = np.ones(q_len) if row_scale is None else np.asarray(row_scale, np.float64)
    out = np.zeros((hq, q_len, d))
    some = seen.any(axis=1)
    for h in range(hq):
        s = (q[h] @ k[h // rep].T) * scale * rs[:, None]
        if slopes is not None:
            s = s - float(slopes[h]) * (origin + i - j)
        s = np.where(seen, s, -np.inf)[some]
        p = np.exp(s - s.max(axis=1, keepdims=True))
        out[h, some] = (p / p.sum(axis=1, keepdims=True)) @ v[h // rep]
    return out


def check_precondition(oracle_out, expected, what: str = "") -> float:
    """The op's fp64 oracle on the rounded inputs returns the expected V rows within 2**-20 in every element."""
    diff = float(np.abs(np.asarray(oracle_out, np.float64) - np.asarray(expected, np.float64)).max())
    assert diff < PRECONDITION, f"{what}: the oracle is {diff:.3e} from the expected V rows (bar 2**-20)"
    return diff


def alibi_slopes(hq: int) -> np.ndarray:
    """The standard slopes 2**(-8 (h+1) / hq) of the head count, with the last head's slope set to 0."""
    sl = np.array([F32(2 ** (-8 * (h + 1) / hq)) for h in range(hq)], F32)
    sl[-1] = 0.0
    return sl


# ---- the cases (hq, hkv, q_len, kv_len, d[, dtype]); shared by the CPU precondition tests and the GPU tests --------------
# Second-generation flash kernel (q_len > 128): 128-row query tiles, 64-key tiles, 1 / 2 / 4 KV runs from 8 / 16 tiles on.
FLASH2 = [(4, 2, 129, 129, 128),       # one row in the second query tile
          (2, 1, 257, 400, 128),       # mask offset 143: no tile multiple
          (8, 2, 300, 300, 128),
          (4, 4, 513, 513, 64),        # 9 KV tiles: two runs, five query tiles (the heavy-first order folds back)
          (2, 2, 200, 1000, 64),       # 16 tiles: four runs
          (2, 1, 130, 1030, 128),      # 17 tiles, four runs, ragged last tile
          (2, 2, 256, 512, 128)]       # every edge on a tile boundary
# One-tile kernel: bf16, head_dim 128, kv_len <= 128, q_len <= 128 (32 query rows per workgroup, 32-key steps).
# (4,1,1,37,128) is listed with the first-generation shapes in the plan of these tests; the dispatch gives it to this kernel.
ONE_TILE = [(3, 1, 1, 1, 128), (4, 4, 17, 17, 128), (2, 1, 33, 128, 128), (8, 2, 70, 100, 128), (2, 1, 128, 128, 128),
            (4, 1, 1, 37, 128)]
# First-generation kernel: q_len <= 128 otherwise (64-row query tiles).  The last two are what the one-tile kernel refuses
# at kv_len <= 128: f16, and head_dim 64.
GEN1 = [(8, 2, 70, 200, 128, "bf16"), (2, 2, 128, 130, 64, "bf16"), (4, 2, 64, 129, 128, "f16"), (2, 2, 65, 193, 64, "bf16"),
        (2, 1, 33, 128, 128, "f16"), (2, 2, 40, 100, 64, "bf16"), (4, 1, 1, 137, 128, "bf16")]
NAIVE = [(2, 1, 40, 75, 128, "f32"), (2, 2, 19, 50, 40, "bf16")]
NAIVE_ENV = (4, 2, 200, 200, 128, "bf16")              # under PYGPUKIT_FLASH_ATTENTION=0
# sdpa_causal_fp8 (bf16, head_dim 128, one kernel for every q_len); (2,1,140,520) adds the two-run split to the listed ones.
FP8 = [(2, 1, 150, 150, 128), (2, 2, 96, 160, 128), (4, 2, 129, 400, 128), (2, 1, 130, 1030, 128), (4, 4, 17, 17, 128),
       (2, 1, 140, 520, 128)]
# sdpa_irope: (…, dtype, smaller causal_offset or None).  kv_len == q_len leaves no smaller offset (the op refuses a negative
# one).  In the last case the smaller offset also moves the split count: 17 tiles of keys, 7 of them seen.
IROPE = [(4, 2, 129, 129, 128, "bf16", None), (2, 1, 257, 400, 128, "bf16", 70), (2, 2, 70, 200, 128, "bf16", 37),
         (2, 2, 200, 500, 64, "f16", 131), (2, 1, 130, 1030, 128, "bf16", 300)]
# sdpa_alibi always runs the flash kernel; one shape each of the three lists above, and one with four KV runs in f16.
ALIBI = [(8, 2, 300, 300, 128, "bf16"), (8, 2, 70, 100, 128, "bf16"), (8, 2, 70, 200, 128, "bf16"), (2, 2, 200, 1000, 64, "f16")]
# Fixed-cache decode: G = 1, 2, 4, 1 query heads per workgroup; four splits at 1024 cache rows, two at 300.
DECODE_HEADS = [(2, 2), (4, 2), (8, 2), (5, 1)]
DECODE_CTX = [(1024, c) for c in (1, 255, 256, 257, 512, 1023, 1024)] + [(300, 299), (300, 300)]
# The five-heads-per-workgroup decode kernel of sdpa_alibi / sdpa_irope_fixed_cache needs splits * (hq / 5) >= 256:
# 8 splits (2048 cache rows) x 32 kv heads.
DECODE_G5 = (160, 32, 2048, 64)                         # hq, hkv, max_seq, d
# paged_attention_v1 (num_seqs, hq, hkv, d, block_size, ctxs); the last one adds a sequence whose second split is empty.
PAGED = [(3, 16, 8, 128, 16, (37, 1, 160)), (2, 8, 8, 64, 8, (17, 64)), (1, 4, 1, 128, 32, (700,)), (5, 2, 2, 64, 4, (3, 9, 1, 12, 7)),
         (2, 16, 2, 128, 16, (2048, 1300)), (2, 4, 2, 128, 16, (600, 5))]
MAX_KV = 2112
