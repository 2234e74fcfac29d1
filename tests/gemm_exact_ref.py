"""Integer-valued operands for exact per-element checks of the dense GEMM family (NumPy only).

A whole-tensor relative error does not see one wrong element, a wrong tile corner or a bias lost on the last column.  Here
every operand is a small integer (times a power-of-two block scale on the fp8 paths), so every fp32 partial sum is exact in
any order and every expected output is exactly representable in the output type: the device result must equal the float64
product word for word, and there is no tolerance to choose.

    bf16 / f16 / fp32:  A in {-1, 0, 1}, W in {-2 .. 2}; W[:, 0] = n % 5 - 2 and A[:, 1] = m % 3 - 1, so that a transposed or
                        row-swapped store cannot pass; bias in {-4 .. 4}, never 0 on the last column.
    fp8 paths:          e4m3 codes of the integers 0 .. 4 (both operands of fp8_nt: 0 .. 2), sparse, with
                        scale_a[m, kb] = (0.5, 1, 2)[(m + kb) % 3]  and  scale_w[nb, kb] = (0.5, 1, 2, 4)[(nb + kb) % 4]:
                        no two neighbouring blocks share a scale, so a scale read from the wrong block changes the result.

Representability (checked for every case in tests/test_gemm_exact_cpu.py): expected == round_to_dtype(expected), and every
unrounded sum stays below 2**24.  bf16 holds the integers up to 256, so the operands get sparser as K grows (density()); on
the fp8 paths the sums are multiples of the smallest scale product and must stay within 256 of those units.

CASES is the table the CPU and GPU files share: one entry per (entry point, dtype, shape, environment) with the dispatch
leaf that gemm_plan must report for it ("GEMM dispatch leaves").
"""

from __future__ import annotations

import functools
import re
from dataclasses import dataclass

import numpy as np

from oracle import cpu_ref as O

F64 = np.float64
NAN_WORD = {"bf16": 0x7FC0, "f16": 0x7E00}
DTYPE_NAME = {"bf16": "bfloat16", "f16": "float16", "f32": "float32"}
SCALE_A = (0.5, 1.0, 2.0)
SCALE_W = (0.5, 1.0, 2.0, 4.0)
FP8_OPS = ("w8a16_nk", "w8a16_kn", "gemv_fp8", "fp8_nt")


# ---- number formats ----------------------------------------------------------------------------------------------------

def to_words(x, dtype: str) -> np.ndarray:
    """Values -> what the device holds: uint16 words for bf16 / f16 (round to nearest even), float32 for f32."""
    x = np.ascontiguousarray(x, np.float32)
    if dtype == "f32":
        return x
    return O.f32_to_bf16_bits(x) if dtype == "bf16" else x.astype(np.float16).view(np.uint16)


def from_words(w, dtype: str) -> np.ndarray:
    if dtype == "f32":
        return np.asarray(w, np.float32)
    w = np.ascontiguousarray(w, np.uint16)
    return O.bf16_bits_to_f32(w) if dtype == "bf16" else w.view(np.float16).astype(np.float32)


def round_to(x, dtype: str) -> np.ndarray:
    """float64 values -> the nearest value of `dtype`, as float64."""
    return from_words(to_words(x, dtype), dtype).astype(F64)


@functools.lru_cache(maxsize=None)
def _int_codes() -> dict:
    """e4m3 code of each integer 0 .. 4 (from the oracle's decode table, as test_gemm_fp8_exact_integers builds them)."""
    table = O.fp8_e4m3_table()
    return {int(v): c for c, v in enumerate(table[:0x7F]) if v == np.floor(v) and v <= 4}


def fp8_encode(x: np.ndarray) -> np.ndarray:
    """Integers -4 .. 4 -> e4m3 codes (sign bit 0x80)."""
    lut = np.array([_int_codes()[i] for i in range(5)], np.uint8)
    return lut[np.abs(x).astype(np.int64)] | np.where(x < 0, 0x80, 0).astype(np.uint8)


# ---- the case table -----------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Case:
    op: str                      # nt, nn, w8a16_nk, w8a16_kn, gemv_fp8, fp8_nt
    dtype: str                   # bf16, f16, f32 (operands and output; the fp8 entry points are bf16)
    m: int
    n: int
    k: int
    leaf: str                    # what gemm_plan must report
    env: tuple = ()              # ((name, value), ...) of PGK_GEMM256 / PGK_GEMM256S; both are unset otherwise
    aligned: bool = True         # False: A starts one element off a 16-byte boundary

    @property
    def bias(self) -> bool:
        return self.op == "nt"   # the only entry point that takes one; every nt case carries it

    def __str__(self) -> str:
        env = "".join(f"-{k[4:]}={v}" for k, v in self.env)
        return f"{self.op}-{self.dtype}-{self.m}x{self.n}x{self.k}{env}{'' if self.aligned else '-unaligned'}-{self.leaf}"


G256 = (("PGK_GEMM256", "1"),)
G128 = (("PGK_GEMM256", "0"),)
LOCKSTEP = (("PGK_GEMM256", "1"), ("PGK_GEMM256S", "0"))
WS_MT = {1: 1, 16: 1, 17: 2, 32: 2, 33: 4, 64: 4, 65: 8, 128: 8}


def _cases() -> list:
    c = []
    # -- nt, fp32 or K % 8 != 0, M <= 8: the GEMV kernels.  fp32 vectors hold 4 elements (K = 100 fast, 101 generic); 16-bit
    #    ones hold 8, so K = 100 is generic there and K = 104 the fast kernel
    for m in range(1, 9):
        c.append(Case("nt", "f32", m, 37, 100, f"gemv_fast_m{m}"))
        for dt in ("bf16", "f16"):
            c.append(Case("nt", dt, m, 37, 104, f"gemv_fast_m{m}"))
    for m in range(1, 9):
        c.append(Case("nt", "f32", m, 37, 101, "gemv_generic"))
    for dt in ("bf16", "f16"):
        c += [Case("nt", dt, 1, 37, 101, "gemv_generic"), Case("nt", dt, 8, 37, 101, "gemv_generic")]
    c += [Case("nt", "bf16", 3, 37, 100, "gemv_generic"), Case("nt", "f16", 3, 37, 100, "gemv_generic")]
    # two trips of a wave (64 lanes x one 16-byte vector) plus a tail of one vector
    c += [Case("nt", "f32", 5, 37, 516, "gemv_fast_m5"), Case("nt", "bf16", 8, 37, 1032, "gemv_fast_m8"),
          Case("nt", "f16", 2, 37, 1032, "gemv_fast_m2")]
    # -- an A that starts one element off a 16-byte boundary keeps K % 8 == 0 shapes on the element-wise kernels
    c += [Case("nt", "bf16", 4, 37, 104, "gemv_generic", aligned=False), Case("nt", "f32", 3, 37, 100, "gemv_generic", aligned=False),
          Case("nt", "f16", 70, 130, 40, "simple_nt", aligned=False), Case("nn", "bf16", 70, 136, 40, "simple_nn", aligned=False)]
    # -- nt, the 64 x 64 x 16 fallback kernel: fp32, or 16 bits with K % 8 != 0
    for dt in ("f32", "bf16", "f16"):
        c += [Case("nt", dt, 9, 130, 33, "simple_nt"), Case("nt", dt, 70, 130, 33, "simple_nt")]
    # -- nt, bf16, M <= 128: the weight-streaming kernel, 256-k tiles (K = 520: two tiles and a tail of 8; 264: one and 8)
    c.append(Case("nt", "bf16", 1, 200, 32776, "wsgemm_mt1"))      # m * k * 2 > 64 KiB keeps one row off the GEMV kernel
    for m, mt in WS_MT.items():
        if m > 1:
            c += [Case("nt", "bf16", m, 200, 520, f"wsgemm_mt{mt}"), Case("nt", "bf16", m, 200, 264, f"wsgemm_mt{mt}")]
    # -- nt, bf16, M > 128, K % 64 == 0, N % 8 == 0: the staged kernels
    c += [Case("nt", "bf16", 129, 136, 192, "gemm128s"), Case("nt", "bf16", 300, 520, 128, "gemm128s")]
    c += [Case("nt", "bf16", 300, 520, 192, "gemm256s", G256), Case("nt", "bf16", 512, 384, 128, "gemm256s_n192", G256),
          Case("nt", "bf16", 257, 192, 64, "gemm256s_n192", G256),
          Case("nt", "bf16", 300, 520, 192, "gemm256_lockstep", LOCKSTEP), Case("nt", "bf16", 512, 384, 128, "gemm256_lockstep", LOCKSTEP)]
    # -- nt, bf16, M > 128, K % 64 != 0: dispatch_mfma (from M > 128 only 128 x 32, 128 x 128 and the 64 x 64 it turns 128 x 64 into)
    c += [Case("nt", "bf16", 200, 100, 72, "mfma_128x32_B_NT"), Case("nt", "bf16", 1024, 2048, 72, "mfma_64x64_B_NT"),
          Case("nt", "bf16", 2048, 2048, 72, "mfma_128x128_B_NT")]
    # -- nt f16, nn f16, nn bf16: every reachable tile of dispatch_mfma.  BN = 64 needs ceil(N/128) < 256 <= ceil(N/64) at one
    #    row block (N = 16328), BN = 128 needs ceil(N/128) >= 256 (N = 32648); K = 72 / 136: one / two 64-k tiles and a tail of 8
    for op, dt, mode in (("nt", "f16", "B_NT"), ("nn", "f16", "B_NN"), ("nn", "bf16", "B_NN")):
        for m, bm in ((20, 32), (50, 64)):
            c += [Case(op, dt, m, 104, 136, f"mfma_{bm}x32_{mode}"), Case(op, dt, m, 16328, 72, f"mfma_{bm}x64_{mode}"),
                  Case(op, dt, m, 32648, 72, f"mfma_{bm}x128_{mode}")]
        c += [Case(op, dt, 200, 104, 136, f"mfma_128x32_{mode}"), Case(op, dt, 1000, 2040, 72, f"mfma_64x64_{mode}"),
              Case(op, dt, 1930, 2040, 72, f"mfma_128x128_{mode}")]
    # -- nn: fp32, or N % 8 != 0
    c += [Case("nn", "f32", 70, 130, 33, "simple_nn"), Case("nn", "bf16", 70, 130, 40, "simple_nn"), Case("nn", "f16", 9, 130, 33, "simple_nn")]
    # -- w8a16_nk: M <= 128 streams the fp8 weight (K = 384: one 256-k tile and half of one, three scale blocks)
    for m, mt in ((16, 1), (20, 2), (50, 4), (100, 8)):
        c.append(Case("w8a16_nk", "bf16", m, 256, 384, f"wsgemm_mt{mt}_fp8"))
    c += [Case("w8a16_nk", "bf16", 300, 256, 256, "mfma_128x32_B_NT_FP8", G128), Case("w8a16_nk", "bf16", 1000, 2048, 256, "mfma_64x64_B_NT_FP8", G128),
          Case("w8a16_nk", "bf16", 1930, 2048, 256, "mfma_128x128_B_NT_FP8", G128),
          Case("w8a16_nk", "bf16", 300, 256, 256, "dequant+gemm256s", G256), Case("w8a16_nk", "bf16", 300, 384, 256, "dequant+gemm256s_n192", G256),
          Case("w8a16_nk", "bf16", 300, 256, 256, "dequant+gemm256_lockstep", LOCKSTEP)]
    # -- w8a16_kn: dispatch_mfma with BN clamped to >= 64 (the only way to 128 x 64)
    c += [Case("w8a16_kn", "bf16", 16, 128, 256, "mfma_32x64_B_KN_FP8"), Case("w8a16_kn", "bf16", 50, 128, 256, "mfma_64x64_B_KN_FP8"),
          Case("w8a16_kn", "bf16", 300, 256, 256, "mfma_128x64_B_KN_FP8"), Case("w8a16_kn", "bf16", 16, 32768, 256, "mfma_32x128_B_KN_FP8"),
          Case("w8a16_kn", "bf16", 50, 32768, 256, "mfma_64x128_B_KN_FP8"), Case("w8a16_kn", "bf16", 1930, 2048, 256, "mfma_128x128_B_KN_FP8")]
    # -- gemv_fp8: passes of <= 8 rows
    for m in range(1, 9):
        c.append(Case("gemv_fp8", "bf16", m, 256, 256, f"gemv_fp8_m{m}"))
    c += [Case("gemv_fp8", "bf16", 9, 256, 256, "gemv_fp8_m8x1+m1"), Case("gemv_fp8", "bf16", 17, 256, 256, "gemv_fp8_m8x2+m1"),
          Case("gemv_fp8", "bf16", 16, 256, 256, "gemv_fp8_m8x2"),
          Case("gemv_fp8", "bf16", 3, 256, 2176, "gemv_fp8_m3")]      # two trips of a wave (64 lanes x 16 codes) and 128 more
    # -- fp8_nt: the 128-tile kernel (ragged M and N), and the 256-tile one (whole tiles by contract)
    c += [Case("fp8_nt", "bf16", 48, 160, 256, "fp8_128"), Case("fp8_nt", "bf16", 300, 520, 384, "fp8_128"),
          Case("fp8_nt", "bf16", 300, 520, 384, "fp8_128", G256),      # forced, but not whole tiles: falls back
          Case("fp8_nt", "bf16", 256, 256, 256, "fp8_128", G128),
          Case("fp8_nt", "bf16", 256, 256, 256, "fp8_256", G256), Case("fp8_nt", "bf16", 512, 768, 384, "fp8_256", G256)]
    return c


CASES = _cases()

# Leaves that no shape reaches, with the argument (also in DESIGN.md):
UNREACHABLE = {
    # bn stops at 64 only with mblocks * ceil(N/128) < 256, and ceil(N/64) <= 2 * ceil(N/128), so mblocks * ceil(N/64) < 512:
    # exactly the condition under which mfma_pick_tile turns 128 x 64 into 64 x 64.  Only B_KN_FP8's clamp of bn = 32 to 64,
    # applied after that line, leaves 128 x 64 standing.
    "mfma_128x64_B_NT", "mfma_128x64_B_NN", "mfma_128x64_B_NT_FP8",
    # that clamp leaves B_KN_FP8 no 32-column tile
    "mfma_32x32_B_KN_FP8", "mfma_64x32_B_KN_FP8", "mfma_128x32_B_KN_FP8",
    # pgk_w8a16_gemm_nk sends M <= 128 to the weight-streaming kernel, so dispatch_mfma only sees it with bm = 128 (or the 64 x 64
    # made from 128 x 64); likewise pgk_gemm_nt in bf16 (in f16 the same tiles are reached from M <= 64)
    "mfma_32x32_B_NT_FP8", "mfma_32x64_B_NT_FP8", "mfma_32x128_B_NT_FP8", "mfma_64x32_B_NT_FP8", "mfma_64x128_B_NT_FP8",
}


def family(leaf: str) -> str:
    """gemv_fp8 beyond 8 rows prints its pass count and the rows of the last pass: one family for whole passes, one with a rest."""
    return re.sub(r"\+m\d$", "+rest", re.sub(r"_m8x\d+", "_m8xP", leaf))


def all_leaves() -> set:
    """Every name gemm_plan can print, up to family()."""
    leaves = {f"gemv_fast_m{m}" for m in range(1, 9)} | {f"gemv_fp8_m{m}" for m in range(1, 9)} | {"gemv_fp8_m8xP", "gemv_fp8_m8xP+rest"}
    leaves |= {"gemv_generic", "simple_nt", "simple_nn", "gemm128s", "fp8_128", "fp8_256"}
    leaves |= {f"wsgemm_mt{mt}{f}" for mt in (1, 2, 4, 8) for f in ("", "_fp8")}
    g256 = ("gemm256s", "gemm256s_n192", "gemm256_lockstep")
    leaves |= set(g256) | {"dequant+" + g for g in g256}
    leaves |= {f"mfma_{bm}x{bn}_{mode}" for bm in (32, 64, 128) for bn in (32, 64, 128) for mode in ("B_NT", "B_NN", "B_NT_FP8", "B_KN_FP8")}
    return leaves


def tile_of(c: Case) -> tuple:
    """(BM, BN, KT) of the kernel behind the case's leaf: the tile a workgroup (for the GEMV kernels: a wave's trip) owns."""
    leaf = c.leaf
    m = re.match(r"mfma_(\d+)x(\d+)_", leaf)
    if m:
        return int(m.group(1)), int(m.group(2)), 64
    if leaf.startswith("wsgemm_mt"):
        return 16 * int(re.match(r"wsgemm_mt(\d)", leaf).group(1)), 64, 256
    if leaf.startswith("gemv_fp8"):
        return 8, 4, 1024
    if leaf.startswith("gemv_fast"):
        return c.m, 4, 256 if c.dtype == "f32" else 512
    if leaf == "gemv_generic":
        return 1, 1, 64
    if leaf.startswith("simple"):
        return 64, 64, 16
    if leaf == "gemm128s":
        return 128, 128, 64
    if leaf == "fp8_128":
        return 128, 128, 128
    if leaf == "fp8_256":
        return 256, 256, 128
    return 256, 192 if leaf.endswith("n192") else 256, 64      # gemm256s, _n192, _lockstep, with or without dequant+


# ---- operands -----------------------------------------------------------------------------------------------------------

def density(c: Case) -> tuple:
    """(fraction of non-zero A, fraction of non-zero W) that keeps 6 sigma of the sums inside the integers bf16 holds.
    Dense pair: var = K dA E[w^2] = 2 K dA (W uniform in -2 .. 2), kept below 1600.  w8a16 / gemv_fp8: units of 0.5, weights
    2 sw in {1, 2, 4, 8} (mean square 21.25), W uniform in +-{1 .. 4} (7.5): var = 160 K dA dW = 480.  fp8_nt: units of 0.25,
    weights 4 sa sw in {1 .. 32} (mean square 149), A and W in +-{1, 2} (2.5 each; one product at the largest scales is already
    128 units, so 3 and 4 stay with the w8a16 paths): var = 930 K dA dW = 230.  The sums of few large terms have heavier tails
    than a Gaussian, hence the wider margin; the representability test is what decides."""
    if c.op not in FP8_OPS:
        return min(2.0 / 3.0, 800.0 / c.k), 1.0
    d = (3.0 / c.k) ** 0.5 if c.op != "fp8_nt" else (0.25 / c.k) ** 0.5
    return d, d


@dataclass(frozen=True)
class Operands:
    case: Case
    a: np.ndarray                # [M, K] integer values (float64)
    w: np.ndarray                # [N, K] integer values (float64), whatever layout the entry point stores
    bias: np.ndarray | None      # [N]
    sa: np.ndarray | None        # [M, K/128] fp8_nt only
    sw: np.ndarray | None        # [ceil(N/128), K/128] fp8 paths
    expected: np.ndarray         # [M, N] float64, exact


def _sparse_ints(rng, shape, dens, hi):
    mag = rng.integers(1, hi + 1, shape)
    sign = rng.integers(0, 2, shape) * 2 - 1
    return (mag * sign * (rng.random(shape) < dens)).astype(F64)


def product(a, w, bias=None, sa=None, sw=None) -> np.ndarray:
    """The float64 product (a BLAS call per 128-k block where scales apply): exact for these operands."""
    if sw is None:
        out = a @ w.T
    else:
        m, k = a.shape
        n = w.shape[0]
        out = np.zeros((m, n), F64)
        for b in range(k // 128):
            part = a[:, b * 128:(b + 1) * 128] @ w[:, b * 128:(b + 1) * 128].T
            part *= np.repeat(sw[:, b], 128)[None, :n]
            if sa is not None:
                part *= sa[:, b:b + 1]
            out += part
    return out if bias is None else out + bias[None, :]


@functools.lru_cache(maxsize=8)
def make(c: Case) -> Operands:
    """Operands and the expected output of a case; computed once and shared (the arrays are read-only)."""
    rng = np.random.default_rng([c.m, c.n, c.k, FP8_OPS.index(c.op) if c.op in FP8_OPS else 7])
    da, dw = density(c)
    m_idx, n_idx = np.arange(c.m), np.arange(c.n)
    bias = sa = sw = None
    if c.op in FP8_OPS:
        a = _sparse_ints(rng, (c.m, c.k), da, 2 if c.op == "fp8_nt" else 1)
        w = _sparse_ints(rng, (c.n, c.k), dw, 2 if c.op == "fp8_nt" else 4)
        w[:, 0] = n_idx % 3 == 0 if c.op == "fp8_nt" else n_idx % 3 + 1      # asymmetric in n, against a sparse A column
        a[:, 1] = m_idx % 2 if c.op == "fp8_nt" else m_idx % 3 - 1           # asymmetric in m, against a sparse W column
        kb = c.k // 128
        sw = np.array(SCALE_W)[(np.arange((c.n + 127) // 128)[:, None] + np.arange(kb)[None, :]) % 4]
        if c.op == "fp8_nt":
            sa = np.array(SCALE_A)[(m_idx[:, None] + np.arange(kb)[None, :]) % 3]
    else:
        a = _sparse_ints(rng, (c.m, c.k), da, 1)
        w = rng.integers(-2, 3, (c.n, c.k)).astype(F64)
        w[:, 0] = n_idx % 5 - 2
        if c.k > 1:
            a[:, 1] = m_idx % 3 - 1
        if c.bias:
            bias = rng.integers(-4, 5, c.n).astype(F64)
            bias[-1] = 3.0
    ops = Operands(c, a, w, bias, sa, sw, product(a, w, bias, sa, sw))
    for x in (ops.a, ops.w, ops.bias, ops.sa, ops.sw, ops.expected):
        if x is not None:
            x.setflags(write=False)
    return ops


def expected_words(c: Case) -> np.ndarray:
    return to_words(make(c).expected, c.dtype)


# ---- mutants: what a wrong kernel would return ---------------------------------------------------------------------------

def chunk_start(c: Case) -> int:
    """An aligned 8-wide K chunk inside the second K tile of the kernel (the first, where K has only one): the first one from
    there on in which A holds anything."""
    kt = tile_of(c)[2]
    k0 = min(kt + 8, (c.k // 8 - 1) * 8) if c.k >= 16 else 0
    a = make(c).a
    for k in list(range(k0, c.k - 7, 8)) + list(range(0, k0, 8)):
        if a[:, k:k + 8].any():
            return k
    return k0


def tail_start(c: Case) -> int:
    """Start of the K tail: what lies beyond the last whole K tile (the last tile itself where K is a whole number of them)."""
    kt = tile_of(c)[2]
    return (c.k - 1) // kt * kt


def mutants(c: Case) -> dict:
    """name -> float64 output of a reference with one planted error.  Every one must differ from the expected output in at
    least one word (tests/test_gemm_exact_cpu.py); bias and scale mutants exist only where the entry point has them."""
    o = make(c)
    e = o.expected
    bm, bn, _ = tile_of(c)
    out = {}

    def without(k0, k1):
        a = o.a.copy()
        a[:, k0:k1] = 0.0
        return product(a, o.w, o.bias, o.sa, o.sw)

    k0 = chunk_start(c)
    out["drop_k_chunk"] = without(k0, k0 + 8)
    out["drop_k_tail"] = without(tail_start(c), c.k)
    if c.m > 1:
        out["shift_rows"] = np.roll(e, 1, axis=0)
    sw_cols = e.copy()
    sw_cols[:, [c.n - 2, c.n - 1]] = e[:, [c.n - 1, c.n - 2]]
    out["swap_columns"] = sw_cols
    if o.bias is not None:
        nb = e.copy()
        nb[:, -1] -= o.bias[-1]
        out["no_bias_on_last_column"] = nb
    if o.sw is not None:
        if o.sw.shape[1] > 1:
            out["neighbour_w_scale_block"] = product(o.a, o.w, o.bias, o.sa, np.roll(o.sw, 1, axis=1))
        if o.sw.shape[0] > 1:
            out["neighbour_w_scale_row_block"] = product(o.a, o.w, o.bias, o.sa, np.roll(o.sw, 1, axis=0))
    if o.sa is not None and o.sa.shape[1] > 1:
        out["neighbour_a_scale_block"] = product(o.a, o.w, o.bias, np.roll(o.sa, 1, axis=1), o.sw)
    t = min(max(min(bm, bn), 8), c.m, c.n)                                   # a square corner of the first tile (8 x 8 at least)
    if t > 1:
        tr = e.copy()
        tr[:t, :t] = e[:t, :t].T
        out["transpose_tile"] = tr
    return out


def suspects(c: Case) -> dict:
    """name -> words of the usual wrong answers, for the failure message of the GPU file."""
    o = make(c)
    e = o.expected
    a = o.a.copy()
    a[:, tail_start(c):] = 0.0
    s = {"the row above": np.roll(e, 1, axis=0), "the row below": np.roll(e, -1, axis=0),
         "the column to the left": np.roll(e, 1, axis=1), "the column to the right": np.roll(e, -1, axis=1),
         "the sum without the last K tile": product(a, o.w, o.bias, o.sa, o.sw), "zero": np.zeros_like(e)}
    if o.bias is not None:
        s["the sum without the bias"] = e - o.bias[None, :]
    return {k: to_words(v, c.dtype) for k, v in s.items()}


def explain(c: Case, got: np.ndarray, want: np.ndarray) -> str:
    """The first dozen wrong (m, n) with their tile coordinates under the plan's BM x BN and what the value equals instead."""
    bm, bn, kt = tile_of(c)
    bad = np.argwhere(got != want)
    lines = [f"{c}: {len(bad)} of {want.size} words differ (tile {bm} x {bn} x {kt})"]
    if not len(bad):
        return lines[0]
    sus = suspects(c)
    for m, n in bad[:12]:
        hits = [name for name, v in sus.items() if v[m, n] == got[m, n]]
        lines.append(f"  ({m}, {n}) tile ({m // bm}, {n // bn}) at ({m % bm}, {n % bn}): expected {from_words(want[m, n], c.dtype).ravel()[0]}, "
                     f"got {from_words(got[m, n], c.dtype).ravel()[0]}" + (f" = {' / '.join(hits)}" if hits else ""))
    rows, cols = np.unique(bad[:, 0]), np.unique(bad[:, 1])
    lines.append(f"  rows {rows[:8].tolist()}{'...' if len(rows) > 8 else ''} ({len(rows)}), columns {cols[:8].tolist()}"
                 f"{'...' if len(cols) > 8 else ''} ({len(cols)})")
    return "\n".join(lines)
