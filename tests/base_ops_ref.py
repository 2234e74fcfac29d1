"""Cases, float64 oracle and per-element error bars of the base op kernels (csrc/ops_elementwise.hip, ops_reduce.hip,
ops_norm_rope.hip).  tests/test_base_ops_cpu.py checks the table, the bars and the planted errors without a device;
tests/test_base_ops_gpu.py runs every case on the kernels.

A case names an op, a dtype, a shape, the operands that sit one element off 16-byte alignment and the dispatch leaf
base_op_plan must report (csrc/base_plan.h).  The oracle works on the values the device holds (inputs rounded to the storage
type first) and EVERY element of every output is compared: as storage words where the result is exact, under a bar otherwise.

Notation: u = 2^-24 (float32 unit roundoff); N = 4 (float32) or 8 (16-bit) elements per 16-byte vector; v the exact value;
h = half an ulp of the output type, 0 / 2^-8 |v| / 2^-11 |v| for float32 / bfloat16 / float16 (float16 also gets 2^-25, half
its subnormal spacing), the convention of tests/audio_ref.py.  A float32 result v' within `bar` of v rounds to storage within
bar + h (|v| + bar); that is what `total_bar` returns.

Word-exact: add, sub, mul (and both in-place forms), relu, relu2, abs, neg, bias add, clamp, where, casts, the whole-array
reductions and sum_axis on integer data, RoPE on the exact data set.  For 16-bit storage the oracle does the float32
operation and then one rounding, as the kernels do.

Bars:
  div, sqrt, rsqrt         2u |v|, 2u |v|, 4u |v|: one or two operations of at most one ulp each, whether or not the compiler
                           rounds them correctly.
  exp log sin cos tanh     LIB_RTOL |v| + LIB_ATOL = 3e-6 |v| + 1e-6, gelu 2e-5 |v| + 2e-6: the bars the fixture tests of
  sigmoid silu gelu        tests/test_gpu_ops.py already meet on the MI355X, on inputs drawn the same way (1.5 x standard normal;
                           |x| + 0.25 for log, sqrt, rsqrt).  exp(0), log(1), sin(0), cos(0), tanh(0), sigmoid(0), silu(0), gelu(0)
                           are planted and asserted exactly (bar 0).
  swiglu, geglu, packed    act(g) up: (LIB_RTOL |act| + LIB_ATOL) |up| for the activation, + u |v| for the product.
  softmax                  y_i = e_i / s, e_i = exp(x_i - m), s = sum_j e_j >= 1.  x_i - m is off by u |x_i - m|, so e_i carries
                           de_i = LIB_ATOL + (LIB_RTOL + u |x_i - m|) e_i (the exp bar, once in the numerator and once per term
                           of the denominator); a sum of n non-negative terms in any order is within n u of itself and the
                           division adds u (2u allowed):  dy_i = de_i / s + y_i (sum_j de_j / s + (n + 2) u).
                           An input of -inf gives e_i = 0 exactly, so y_i = 0 with bar 0.
  rmsnorm                  out = v inv g, inv = 1 / sqrt(ss / n + eps), ss = sum v^2.  The squares and the sum in any order:
                           (n + 1) u of ss (all terms positive); / n and + eps: u each; the square root halves the relative
                           error of its argument and adds 2u, the reciprocal 2u: inv is within (n / 2 + 5.5) u.  Two products:
                           2u.  Bar (n / 2 + 8) u |v|.  With a residual, v = fl(x + r) is off by u, which reaches the numerator
                           once and inv once more: (n / 2 + 10) u |v|.
  layernorm (two pass)     mean' = fl(sum x) / n is off by dm = (n - 1) u mean|x| + u |mean|; d_j = x_j - mean' by dm + u |d_j|;
                           var = sum d^2 / n by dvar = 2 dm mean|d| + dm^2 + (n + 4) u var; inv = 1 / sqrt(var + eps) relatively by
                           r = dvar / (2 (var + eps)) + 5 u; out_j = d_j inv g_j + b_j by
                           |g_j| inv (dm + u |d_j|) + |d_j inv g_j| (r + 3 u) + u |out_j|.
  RoPE (random data)       x0 c - x1 s and x1 c + x0 s: two products and one add, each within u:
                           2u (|x0 c| + |x1 s|), resp. 2u (|x1 c| + |x0 s|).
No constant here is fitted to what a kernel returns; MEASURED (below) records how much of each bar the two float32 NumPy
emulations use on this table, for the record only.

Reductions with no bar: `sum` / `mean` / sum_axis run on integers in [-2, 2] whose running sums stay below 2^24 and whose
total is a small planted integer representable in the output type, so every summation order is exact; `mean` multiplies the
float32 sum once by float32(1 / n), reproduced here.  The planted error "mean divided by n - 1" moves the result by 1 / n of
itself, so it is only applicable where that is at least two ulps of the output type (every n in float32, n <= 64 in bfloat16,
n <= 512 in float16).

Wrap cases: one per kernel template and dtype.  The flat vector kernels size their grid from n / N + 1 vectors, so
n = 2048 256 N + N + 3 is the smallest n at which one whole vector (and a 3-element tail) is left for the second trip of the
grid-stride loop; the inequality base_op_grid(...) 256 N < n already holds from 2048 256 N + 1, where only the scalar tail is
touched.  The scalar leaf uses n = 2048 256 + 5.
"""

from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass

import numpy as np

U = 2.0 ** -24
HALF_ULP = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}
TINY = {"f32": 0.0, "bf16": 0.0, "f16": 2.0 ** -25}
NVEC = {"f32": 4, "bf16": 8, "f16": 8}
ITEM = {"f32": 4, "bf16": 2, "f16": 2, "u8": 1}
DTYPE_NAME = {"f32": "float32", "bf16": "bfloat16", "f16": "float16", "u8": "uint8"}
DTYPES = ("f32", "f16", "bf16")
GUARD_WORD = {"f32": 0x7FC12345, "bf16": 0x7FC5, "f16": 0x7E55, "u8": 0xA5}         # NaN patterns (a byte for cond)
EW_CAP, RD_CAP, BLOCK = 2048, 1024, 256
LIB_RTOL, LIB_ATOL, GELU_RTOL, GELU_ATOL = 3e-6, 1e-6, 2e-5, 2e-6
EPS = float(np.float32(1e-5))          # what the entry points receive
GELU_A, GELU_B = float(np.float32(0.7978845608)), float(np.float32(0.044715))

ACT_CODES = {"silu": 0, "gelu": 1, "sigmoid": 2, "tanh": 3, "relu2": 4, "exp": 5, "log": 6, "relu": 7, "sin": 8, "cos": 9,
             "sqrt": 10, "rsqrt": 11, "abs": 12, "neg": 13}
ACT_EXACT = ("relu2", "relu", "abs", "neg")
ACT_POSITIVE = ("log", "sqrt", "rsqrt")
EXACT_POINT = {"exp": (0.0, 1.0), "log": (1.0, 0.0), "sin": (0.0, 0.0), "cos": (0.0, 1.0), "tanh": (0.0, 0.0),
               "sigmoid": (0.0, 0.5), "silu": (0.0, 0.0), "gelu": (0.0, 0.0)}
BINARY_CODES = {"add": 0, "sub": 1, "mul": 2, "div": 3, "add_inplace": 0, "mul_inplace": 2}
REDUCE_CODES = {"sum": 0, "mean": 1, "max": 2, "min": 3}
NORM_MODES = ("rmsnorm", "rmsnorm_residual", "layernorm")
CAST_PAIRS = (("f32", "bf16"), ("f32", "f16"), ("bf16", "f32"), ("f16", "f32"), ("bf16", "f16"), ("f16", "bf16"))
LEAVES = {"ew_vec", "ew_scalar", "row_vec", "row_scalar", "norm_wave", "norm_block", "cast_x4", "rope_pairs", "ew_stride",
          "reduce_tree"}
PLAN_OP = {"binary": "binary", "act": "activation", "glu": "glu", "glu_packed": "glu_packed", "bias_add": "bias_add",
           "cast": "cast", "rope": "rope", "clamp": "clamp", "where": "where", "reduce": "reduce"}
# measured on the float32 cases of this table with the two float32 NumPy emulations (test_base_ops_cpu.py recomputes them):
# the largest fraction of its bar that any element uses, per family.  In 16-bit storage the half ulp of the output dominates
# and an element can sit anywhere inside it, so the fraction there is close to 1 by construction.  The kernels on an MI355X
# use, in float32: div 0.50, sqrt 0.49, rsqrt 0.36, lib 0.04, gelu 0.03, glu 0.05, softmax 0.005, rmsnorm 0.20,
# rmsnorm_residual 0.17, layernorm 0.23, rope 0.79.
MEASURED = {"div": 0.50, "sqrt": 0.49, "rsqrt": 0.36, "lib": 0.05, "gelu": 0.05, "glu": 0.06, "softmax": 0.01, "rmsnorm": 0.23,
            "rmsnorm_residual": 0.26, "layernorm": 0.23, "rope": 0.86}


# ---- storage formats ----------------------------------------------------------------------------------------------------------
def bf16_bits(x) -> np.ndarray:
    """float32 -> bfloat16 words, round to nearest even; every NaN becomes 0x7FC0."""
    x = np.ascontiguousarray(x, np.float32)
    w = x.view(np.uint32).astype(np.uint64)
    out = ((w + 0x7FFF + ((w >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), out)


def to_words(x, dt: str) -> np.ndarray:
    """Storage words of x (float32 values) rounded once to `dt`; NaN canonical."""
    x = np.ascontiguousarray(x, np.float32)
    if dt == "bf16":
        return bf16_bits(x)
    with np.errstate(over="ignore"):
        if dt == "f16":
            return canonical(x.astype(np.float16).view(np.uint16), dt)
    return canonical(x.view(np.uint32).copy(), dt)


def from_words(w, dt: str) -> np.ndarray:
    w = np.ascontiguousarray(w)
    if dt == "bf16":
        return (w.astype(np.uint32) << 16).view(np.float32)
    if dt == "f16":
        return w.view(np.float16).astype(np.float32)
    return w.view(np.float32).copy()


def canonical(w, dt: str) -> np.ndarray:
    """Words with every NaN replaced by one pattern: NaN is compared as "is NaN"."""
    w = np.ascontiguousarray(w)
    nan = np.isnan(from_words(w, dt))
    return np.where(nan, w.dtype.type({"f32": 0x7FC00000, "bf16": 0x7FC0, "f16": 0x7E00}[dt]), w)


def rounded(x, dt: str) -> np.ndarray:
    """The float32 value the device holds for x stored as `dt`."""
    return from_words(to_words(x, dt), dt)


def total_bar(v, bar, dt: str) -> np.ndarray:
    v, bar = np.asarray(v, np.float64), np.asarray(bar, np.float64)
    extra = HALF_ULP[dt] * (np.abs(v) + bar) + TINY[dt]
    return np.where(bar > 0, bar + extra, 0.0)          # bar 0: a planted exact point, no rounding either


# ---- cases --------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    fam: str
    op: str
    dtype: str
    shape: tuple
    mis: tuple = ()              # operands that start one element past a 16-byte boundary
    leaf: str | None = None      # what base_op_plan must say (None: the launcher has one kernel and no plan entry)
    wrap: bool = False
    extra: tuple = ()            # cast: (destination dtype,); rope: (table dtype, data set); max / min: (index of the extreme,)

    def __str__(self) -> str:
        s = f"{self.fam}-{self.op}-{self.dtype}-" + "x".join(str(d) for d in self.shape)
        s += "".join(f"-{e}" for e in self.extra)
        s += ("-off_" + "_".join(self.mis)) if self.mis else ""
        return s + ("-wrap" if self.wrap else "")

    @property
    def n(self) -> int:
        return int(np.prod(self.shape))


def operands(c: Case) -> dict:
    """name -> (dtype, shape, is_output) of every device operand, in the order of the entry point."""
    dt, sh = c.dtype, c.shape
    if c.fam == "binary":
        if c.op.endswith("_inplace"):
            return {"a": (dt, sh, True), "b": (dt, sh, False)}
        return {"a": (dt, sh, False), "b": (dt, sh, False), "c": (dt, sh, True)}
    if c.fam == "act":
        return {"x": (dt, sh, False), "y": (dt, sh, True)}
    if c.fam == "glu":
        return {"g": (dt, sh, False), "u": (dt, sh, False), "o": (dt, sh, True)}
    if c.fam == "glu_packed":
        return {"gu": (dt, (sh[0], 2 * sh[1]), False), "o": (dt, sh, True)}
    if c.fam == "bias_add":
        return {"out": (dt, sh, True), "bias": (dt, (sh[1],), False)}
    if c.fam == "cast":
        return {"src": (dt, sh, False), "dst": (c.extra[0], sh, True)}
    if c.fam == "norm":
        d = {"x": (dt, sh, False)}
        if c.op == "rmsnorm_residual":
            d["res"] = (dt, sh, False)
        d["gamma"] = (dt, (sh[1],), False)
        if c.op == "layernorm":
            d["beta"] = (dt, (sh[1],), False)
        d["out"] = (dt, sh, True)
        return d
    if c.fam == "rope":
        s, hq, hk, d = sh
        return {"q": (dt, (s, hq, d), True), "k": (dt, (s, hk, d), True), "cos": (c.extra[0], (s, d), False), "sin": (c.extra[0], (s, d), False)}
    if c.fam == "reduce":
        return {"x": (dt, sh, False), "out": (dt, (1,), True)}
    if c.fam == "softmax":
        return {"x": (dt, sh, False), "y": (dt, sh, True)}
    if c.fam == "sum_axis":
        return {"x": (dt, sh, False), "out": (dt, (sh[1] if c.op == "axis0" else sh[0],), True)}
    if c.fam == "clamp":
        return {"x": (dt, sh, False), "y": (dt, sh, True)}
    assert c.fam == "where", c.fam
    return {"cond": ("u8", sh, False), "a": (dt, sh, False), "b": (dt, sh, False), "y": (dt, sh, True)}


def plan_args(c: Case):
    """(op, n_or_rows, features) for base_op_plan / base_op_grid, or None where the launcher has no plan entry."""
    if c.fam == "norm":
        return c.op, c.shape[0], c.shape[1]
    if c.fam in ("glu_packed", "bias_add"):
        return PLAN_OP[c.fam], c.shape[0], c.shape[1]
    if c.fam == "rope":
        s, hq, hk, d = c.shape
        return "rope", s * (hq + hk), d
    if c.fam in PLAN_OP:
        return PLAN_OP[c.fam], c.n, 1
    return None


def wrap_work(c: Case):
    """(work items the grid-stride loop covers, items per block): the case wraps when grid * per_block < items."""
    N = NVEC[c.dtype]
    if c.fam in ("binary", "act", "glu"):
        return (c.n, BLOCK * N) if c.leaf == "ew_vec" else (c.n, BLOCK)
    if c.fam in ("glu_packed", "bias_add"):
        return (c.n, BLOCK * N) if c.leaf == "row_vec" else (c.n, BLOCK)
    if c.fam == "cast":
        return c.n, BLOCK * 4
    if c.fam == "rope":
        s, hq, hk, d = c.shape
        return s * (hq + hk) * (d // 2), BLOCK
    return c.n, BLOCK          # clamp, where, reduce


def _flat_leaf(mis) -> str:
    return "ew_scalar" if mis else "ew_vec"


def _row_leaf(features: int, dt: str, mis) -> str:
    return "row_scalar" if mis or features % NVEC[dt] else "row_vec"


def _norm_leaf(features: int, dt: str, mis) -> str:
    N = NVEC[dt]
    return "norm_wave" if not mis and features % N == 0 and features <= 64 * N * 8 else "norm_block"


def _build_cases() -> list:
    cs = []
    for dt in DTYPES:
        N = NVEC[dt]
        ns = (1, N - 1, N, N + 1, 256 * N + 3)
        wrap_vec, wrap_scalar = EW_CAP * BLOCK * N + N + 3, EW_CAP * BLOCK + 5
        # flat elementwise: every op code at every n on the vector leaf, and on the scalar leaf with each operand off in turn
        for fam, ops_, names in (("binary", tuple(BINARY_CODES), ("a", "b", "c")), ("act", tuple(ACT_CODES), ("x", "y")),
                                 ("glu", ("swiglu", "geglu"), ("g", "u", "o"))):
            for op in ops_:
                who = tuple(n_ for n_ in names if not (op.endswith("_inplace") and n_ == "c"))
                for n in ns:
                    cs.append(Case(fam, op, dt, (n,), (), "ew_vec"))
                    cs += [Case(fam, op, dt, (n,), (m,), "ew_scalar") for m in who]
            first = ops_[3] if fam == "binary" else ops_[0]          # div / silu / swiglu: one wrap per template and dtype
            cs.append(Case(fam, first, dt, (wrap_vec,), (), "ew_vec", True))
            cs.append(Case(fam, first, dt, (wrap_scalar,), (names[0],), "ew_scalar", True))
        # row-structured elementwise
        for fam, ops_, names in (("glu_packed", ("silu", "gelu"), ("gu", "o")), ("bias_add", ("add",), ("out", "bias"))):
            for op in ops_:
                for rows in (1, 3):
                    for f in (N, N + 1, 3 * N):
                        cs.append(Case(fam, op, dt, (rows, f), (), _row_leaf(f, dt, ())))
                cs += [Case(fam, op, dt, (3, 3 * N), (m,), "row_scalar") for m in names]
            rows_v = EW_CAP * BLOCK // 3 + 1                          # rows * 3 vectors just above 2048 * 256
            rows_s = EW_CAP * BLOCK // (N + 1) + 1
            cs.append(Case(fam, ops_[0], dt, (rows_v, 3 * N), (), "row_vec", True))
            cs.append(Case(fam, ops_[0], dt, (rows_s, N + 1), (), "row_scalar", True))
        # norms
        for op in NORM_MODES:
            names = tuple(k for k in operands(Case("norm", op, dt, (1, N))))
            for f in (1, N, 64 * N, 64 * N + N, 64 * N * 8, 64 * N * 8 + N, 255, 256, 257, 3 * N + 1):
                for rows in (1, 4, 5):
                    cs.append(Case("norm", op, dt, (rows, f), (), _norm_leaf(f, dt, ())))
            cs += [Case("norm", op, dt, (4, 64 * N), (m,), "norm_block") for m in names]
        # rope
        for d in (2, 64, 128):
            for hq, hk in ((1, 1), (8, 2), (3, 0)):
                for table in dict.fromkeys(("f32", dt)):
                    for data in ("exact", "random"):
                        cs.append(Case("rope", "rope", dt, (3, hq, hk, d), (), "rope_pairs", False, (table, data)))
        for table in dict.fromkeys(("f32", dt)):
            cs.append(Case("rope", "rope", dt, (700, 8, 4, 128), (), "rope_pairs", True, (table, "exact")))
        # whole-array reductions
        P = RD_CAP * BLOCK
        for n in (1, 63, 64, 65, 255, 256, 257, P - 1, P, P + 1, 2 * P + 7):
            for op in ("sum", "mean"):
                cs.append(Case("reduce", op, dt, (n,), (), "reduce_tree", n > P))
            for op in ("max", "min"):
                for at in sorted({i for i in (0, 255, 256, P, n - 1) if i < n}):
                    cs.append(Case("reduce", op, dt, (n,), (), "reduce_tree", n > P, (at,)))
        # softmax, sum_axis
        for rows in (1, 3, 7):
            for n in (1, 255, 256, 257, 1000):
                cs.append(Case("softmax", "softmax", dt, (rows, n)))
                cs += [Case("sum_axis", ax, dt, (rows, n)) for ax in ("axis0", "axis1")]
        # clamp, where
        for fam in ("clamp", "where"):
            cs += [Case(fam, fam, dt, (n,), (), "ew_stride") for n in ns]
            cs.append(Case(fam, fam, dt, (RD_CAP * BLOCK + 1,), (), "ew_stride", True))
    for src, dst in CAST_PAIRS:
        cs += [Case("cast", "cast", src, (n,), (), "cast_x4", False, (dst,)) for n in (1, 3, 4, 5, 1027)]
        cs += [Case("cast", "cast", src, (1027,), (m,), "cast_x4", False, (dst,)) for m in ("src", "dst")]
        cs.append(Case("cast", "cast", src, (EW_CAP * BLOCK * 4 + 4 + 3,), (), "cast_x4", True, (dst,)))
    return cs


CASES = _build_cases()


def groups() -> dict:
    """Cases grouped for the test ids: one group per family, op and dtype; every wrap case on its own."""
    g: dict = {}
    for c in CASES:
        key = str(c) if c.wrap else f"{c.fam}-{c.op}-{c.dtype}" + (f"-{c.extra[0]}" if c.fam == "cast" else "")
        g.setdefault(key, []).append(c)
    return g


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def _rng(c: Case, salt: str = "") -> np.random.Generator:
    return np.random.default_rng(zlib.crc32((str(c) + salt).encode()))


def cast_table() -> np.ndarray:
    """Special values of the casts, as float32 (then rounded to the source type of the case)."""
    t = [0.0, -0.0, np.inf, -np.inf, np.nan,
         3.4028235e38, -3.4028235e38,                    # largest float32: inf in both 16-bit types
         3.3895314e38, -3.3895314e38,                    # largest bfloat16: inf in float16
         65504.0, -65504.0,                              # largest float16: 65536 in bfloat16
         65519.0, 65520.0, -65519.0, -65520.0,           # float16: the last value that rounds to 65504, the first to inf
         1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -20,      # bfloat16 ties (to even: down, up) and just above
         1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 3 * 2.0 ** -11), 1 + 2.0 ** -11 + 2.0 ** -22,   # float16 ties and just above
         2.0 ** -14, 2.0 ** -15, 1.5 * 2.0 ** -15, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 3 * 2.0 ** -25, -(2.0 ** -24),
         -(2.0 ** -25), 6.0e-8, 1.0e-5, 1.0e-6, 0.75 * 2.0 ** -14, 2.0 ** -26]      # float16 results that are subnormal (or 0)
    return np.array(t, np.float32)


def _int_data(rng, n: int, target: int) -> np.ndarray:
    """n integers in [-2, 2] with sum `target`; the last one is not 0."""
    if n == 1:
        return np.array([float(target)], np.float32)
    x = rng.integers(-2, 3, n).astype(np.int64)
    x[-1] = 1 if target >= 0 else -1
    d = int(x.sum()) - target
    pool = np.flatnonzero((x[:-1] > -2) if d > 0 else (x[:-1] < 2))
    k = abs(d)
    while k:                                           # a few passes where one unit per element is not enough (tiny n)
        take = pool[:k]
        x[take] -= 1 if d > 0 else -1
        k -= take.size
        pool = np.flatnonzero((x[:-1] > -2) if d > 0 else (x[:-1] < 2))
        assert pool.size or not k, (n, target)
    assert int(x.sum()) == target and np.abs(x).max() <= 2
    return x.astype(np.float32)


def _target(n: int, i: int = 0) -> int:
    """Planted total of a row: small, odd, alternating in sign, different per row, reachable with n elements in [-2, 2]."""
    t = min(37 + 6 * i, 2 * n - 1 if n > 1 else 2)
    return t if i % 2 == 0 else -t


NORM_SCALE = (1.0, 2.0 ** -8, 4.0, 8.0, 16.0)       # row 1: mean square of the order of eps; rows differ by powers of two


def _norm_row_kinds(rows: int):
    return (1,) if rows == 1 else tuple(range(rows))


@functools.lru_cache(maxsize=6)
def inputs(c: Case) -> dict:
    """name -> float32 array of the values the device holds (already rounded to the operand's storage type); for `cond` uint8."""
    rng = _rng(c)
    dt, N = c.dtype, NVEC[c.dtype]
    r = lambda x, t=dt: rounded(np.asarray(x, np.float32), t)      # noqa: E731
    if c.fam == "binary":
        return {"a": r(rng.standard_normal(c.shape)), "b": r(rng.standard_normal(c.shape) + 3.0)}
    if c.fam in ("act", "glu"):
        x = rng.standard_normal(c.shape) * 1.5
        act = c.op if c.fam == "act" else ("silu" if c.op == "swiglu" else "gelu")
        if act in ACT_POSITIVE:
            x = np.abs(r(x)) + r(np.full(c.shape, 0.25))
        x = r(x)
        if act in ("relu", "relu2"):
            x = np.abs(x) * np.where(np.arange(c.n) % 2, -1.0, 1.0).astype(np.float32)      # both branches at every n > 1
        if act in EXACT_POINT and c.n >= N:
            x[0] = EXACT_POINT[act][0]
        if c.fam == "act":
            return {"x": x}
        return {"g": x, "u": r(rng.standard_normal(c.shape))}
    if c.fam == "glu_packed":
        rows, inter = c.shape
        g = r(rng.standard_normal(c.shape) * 1.5)
        g[0, 0] = 0.0
        up = r(rng.standard_normal(c.shape) * 16.0)               # the up half is 16 x larger: a wrong half or stride shows
        return {"gu": np.ascontiguousarray(np.concatenate([g, up], axis=1))}
    if c.fam == "bias_add":
        return {"out": r(rng.standard_normal(c.shape)), "bias": r(np.arange(1, c.shape[1] + 1) * 0.25 + rng.standard_normal(c.shape[1]))}
    if c.fam == "cast":
        x = rng.standard_normal(c.shape) * np.exp2(rng.integers(-12, 12, c.shape))
        t = cast_table()
        if c.n >= t.size:
            x[:t.size] = t
            x[-t.size:] = t[::-1]                                   # and once more in the tail of the array
        with np.errstate(over="ignore"):
            return {"src": r(x)}
    if c.fam == "norm":
        rows, f = c.shape
        kinds = _norm_row_kinds(rows)
        x = rng.standard_normal(c.shape)
        for i, kind in enumerate(kinds):
            x[i] *= NORM_SCALE[kind]
            if c.op == "layernorm" and kind == 2:
                x[i] = 100.0 + rng.standard_normal(f)               # mean 100, deviation 1
        d = {"x": r(x), "gamma": r(1.0 + 0.5 * np.cos(np.arange(f) * 0.7) + 0.1 * rng.standard_normal(f))}
        if c.op == "rmsnorm_residual":
            d["res"] = r(rng.standard_normal(c.shape) * np.array([NORM_SCALE[k] for k in kinds])[:, None])
        if c.op == "layernorm":
            d["beta"] = r(0.5 * np.sin(np.arange(f) * 0.3) + 0.1 * rng.standard_normal(f))
        return d
    if c.fam == "rope":
        s, hq, hk, d = c.shape
        table, data = c.extra
        half = d // 2
        cos = np.full((s, d), np.nan, np.float32)                  # the upper half of every row must never be read
        sin = np.full((s, d), np.nan, np.float32)
        if data == "exact":
            cos[:, :half] = rng.choice(np.array([0.0, 1.0, -1.0, 0.5, -0.5], np.float32), (s, half))
            sin[:, :half] = rng.choice(np.array([0.0, 1.0, -1.0, 0.5, -0.5], np.float32), (s, half))
            sin[:, 0] = np.where(np.arange(s) % 2, 1.0, -0.5)       # never 0 in column 0, and different from row to row
            q, k = rng.integers(-8, 9, (s, hq, d)).astype(np.float32), rng.integers(-8, 9, (s, hk, d)).astype(np.float32)
            q[:, :, 0], q[:, :, half] = 3.0, 5.0
            if hk:
                k[:, :, 0], k[:, :, half] = 7.0, 2.0
        else:
            ang = rng.uniform(0.3, 1.2, (s, half))                  # cos and sin both well away from 0
            cos[:, :half], sin[:, :half] = np.cos(ang), np.sin(ang)
            q, k = rng.standard_normal((s, hq, d)), rng.standard_normal((s, hk, d))
        return {"q": r(q), "k": r(k), "cos": r(cos, table), "sin": r(sin, table)}
    if c.fam == "reduce":
        n = c.n
        if c.op in ("sum", "mean"):
            return {"x": _int_data(rng, n, _target(n))}
        x = r(rng.uniform(-4.0, 4.0, n))
        x[c.extra[0]] = 8.0 if c.op == "max" else -8.0
        return {"x": x}
    if c.fam == "softmax":
        rows, n = c.shape
        x = rng.standard_normal(c.shape) * 1.5
        x[:, -1] = x.max(axis=1) + 0.5                              # the last element carries the largest term of the sum
        if rows > 1:
            x[1] += 1e4
        if rows > 2:
            x[2] -= 1e4
        if rows > 3 and n > 2:
            x[3, 0::3][:-1] = -np.inf
            x[3, -1] = 2.0
        if n > 2:
            x[0, 1] = -np.inf                                       # every case has a row with -inf entries
        return {"x": r(x)}
    if c.fam == "sum_axis":
        rows, n = c.shape
        return {"x": np.stack([_int_data(rng, n, _target(n, i)) for i in range(rows)])}
    if c.fam == "clamp":
        x = r(rng.standard_normal(c.shape) * 1.5)
        if c.n >= N:
            x[0], x[1], x[2] = -1.0, 0.5, -0.0
        return {"x": x}
    assert c.fam == "where", c.fam
    return {"cond": rng.choice(np.array([0, 1, 2, 255], np.uint8), c.shape), "a": r(rng.standard_normal(c.shape)),
            "b": r(rng.standard_normal(c.shape) + 5.0)}


CLAMP_LO, CLAMP_HI = -1.0, 0.5


# ---- arithmetic ---------------------------------------------------------------------------------------------------------------
def sum_seq(x, F):
    return np.cumsum(np.asarray(x, F), axis=-1, dtype=F)[..., -1]


def sum_pairwise(x, F):
    x = np.asarray(x, F)
    while x.shape[-1] > 1:
        if x.shape[-1] % 2:
            x = np.concatenate([x, np.zeros(x.shape[:-1] + (1,), F)], axis=-1)
        x = (x[..., 0::2] + x[..., 1::2]).astype(F)
    return x[..., 0]


def sum_exact(x, F):
    return np.asarray(x, np.float64).sum(axis=-1).astype(F)


def act_fn(name: str, x, F):
    x = np.asarray(x, F)
    one, half = F(1.0), F(0.5)
    with np.errstate(all="ignore"):
        if name == "silu":
            return x / (one + np.exp(-x))
        if name == "gelu":
            return x * half * (one + np.tanh(F(GELU_A) * (x + F(GELU_B) * x * x * x)))
        if name == "sigmoid":
            return one / (one + np.exp(-x))
        if name == "relu2":
            t = np.maximum(x, F(0.0))
            return t * t
        if name == "relu":
            return np.maximum(x, F(0.0))
        if name == "rsqrt":
            return one / np.sqrt(x)
        if name == "neg":
            return -x
        return {"tanh": np.tanh, "exp": np.exp, "log": np.log, "sin": np.sin, "cos": np.cos, "sqrt": np.sqrt, "abs": np.abs}[name](x)


def act_bar(name: str, v):
    v = np.abs(np.asarray(v, np.float64))
    if name in ACT_EXACT:
        return np.zeros_like(v)
    if name == "sqrt":
        return 2 * U * v
    if name == "rsqrt":
        return 4 * U * v
    if name == "gelu":
        return GELU_RTOL * v + GELU_ATOL
    return LIB_RTOL * v + LIB_ATOL


def _shift(x):
    """What a kernel that reads element i + 1 for element i sees (flat, wrapping at the end)."""
    return np.roll(np.asarray(x).reshape(-1), -1).reshape(np.shape(x))


def compute(c: Case, ins: dict, F=np.float64, summ=sum_exact, mut: str | None = None) -> dict:
    """name -> array (type F) of every output of the case, computed in arithmetic F with sums by `summ`.  `mut` plants one error."""
    f = lambda a: np.asarray(a, F)      # noqa: E731
    if mut == "shift_one":
        ins = {k: (_shift(v) if k not in ("gamma", "beta", "bias", "cos", "sin") else v) for k, v in ins.items()}
    with np.errstate(all="ignore"):
        if c.fam == "binary":
            a, b = f(ins["a"]), f(ins["b"])
            code = BINARY_CODES[c.op]
            out = (a + b, a - b, a * b, a / b)[code]
            return {"a" if c.op.endswith("_inplace") else "c": out}
        if c.fam == "act":
            return {"y": act_fn(c.op, ins["x"], F)}
        if c.fam == "glu":
            return {"o": act_fn("silu" if c.op == "swiglu" else "gelu", ins["g"], F) * f(ins["u"])}
        if c.fam == "glu_packed":
            inter = c.shape[1]
            gu = f(ins["gu"])
            return {"o": act_fn(c.op, gu[:, :inter], F) * gu[:, inter:]}
        if c.fam == "bias_add":
            b = f(ins["bias"])
            return {"out": f(ins["out"]) + (np.roll(b, 1) if mut == "neighbour_column" else b)[None, :]}
        if c.fam == "cast":
            return {"dst": f(ins["src"])}
        if c.fam == "norm":
            return {"out": _norm(c, ins, F, summ, mut)}
        if c.fam == "rope":
            return _rope(c, ins, F, mut)
        if c.fam == "reduce":
            x = f(ins["x"])
            if mut == "ignore_last" and x.size > 1:
                x = x[:-1]
            if c.op == "max":
                return {"out": x.max(keepdims=True)}
            if c.op == "min":
                return {"out": x.min(keepdims=True)}
            s = np.float32(summ(x, F))
            if c.op == "sum":
                return {"out": np.array([s], F)}
            n = c.n - 1 if mut == "mean_n_minus_1" else c.n
            return {"out": np.array([s * (np.float32(1.0) / np.float32(n))], np.float32).astype(F)}      # the kernel's one float32 multiply
        if c.fam == "softmax":
            x = f(ins["x"])
            if mut == "drop_last" and x.shape[1] > 1:
                m = x[:, :-1].max(axis=1, keepdims=True)
            else:
                m = x.max(axis=1, keepdims=True)
            if mut == "no_max_subtraction":
                m = np.zeros_like(m)
            e = np.exp((x - m).astype(F)).astype(F)
            s = summ(e[:, :-1] if mut == "drop_last" and x.shape[1] > 1 else e, F)
            return {"y": (e / np.asarray(s, F)[:, None]).astype(F)}
        if c.fam == "sum_axis":
            x = f(ins["x"])
            if mut == "drop_last":
                x = x[:, :-1] if c.op == "axis1" else x[:-1]
            return {"out": summ(x if c.op == "axis1" else np.ascontiguousarray(x.T), F) if x.size else np.zeros(c.shape[1 if c.op == "axis0" else 0], F)}
        if c.fam == "clamp":
            return {"y": np.minimum(np.maximum(f(ins["x"]), F(CLAMP_LO)), F(CLAMP_HI))}
        assert c.fam == "where", c.fam
        return {"y": np.where(ins["cond"] != 0, f(ins["a"]), f(ins["b"]))}


def _norm(c: Case, ins: dict, F, summ, mut):
    n = c.shape[1]
    x = np.asarray(ins["x"], F)
    g = np.asarray(ins["gamma"], F)
    eps = F(0.0) if mut == "no_eps" else F(EPS)
    if mut == "neighbour_column":
        g = np.roll(g, 1)
    if c.op == "rmsnorm_residual" and mut != "no_residual":
        x = (x + np.asarray(ins["res"], F)).astype(F)
    if c.op != "layernorm":
        ms = (summ((x * x).astype(F), F) / F(n)).astype(F)
        inv = (F(1.0) / np.sqrt((ms + eps).astype(F))).astype(F)
        if mut == "previous_row_statistic":
            inv = np.roll(inv, 1)
        return (x * inv[:, None] * g[None, :]).astype(F)
    b = np.asarray(ins["beta"], F)
    if mut == "neighbour_column":
        b = np.roll(b, 1)
    mean = (summ(x, F) / F(n)).astype(F)
    d = (x - mean[:, None]).astype(F)
    var = (summ(((x * x) if mut == "variance_without_mean" else (d * d)).astype(F), F) / F(n)).astype(F)
    inv = (F(1.0) / np.sqrt((var + eps).astype(F))).astype(F)
    if mut == "previous_row_statistic":
        inv, mean = np.roll(inv, 1), np.roll(mean, 1)
        d = (x - mean[:, None]).astype(F)
    return (d * inv[:, None] * g[None, :] + b[None, :]).astype(F)


def _rotate(x, cs, sn, F, pairs_adjacent=False):
    """x [..., D] rotated by the table row cs, sn [..., D / 2] (broadcast over heads)."""
    half = x.shape[-1] // 2
    out = x.copy()
    if pairs_adjacent:                                           # the planted error: pairs (d, d + 1)
        x0, x1 = x[..., 0::2], x[..., 1::2]
        out[..., 0::2] = (x0 * cs).astype(F) - (x1 * sn).astype(F)
        out[..., 1::2] = (x1 * cs).astype(F) + (x0 * sn).astype(F)
        return out
    x0, x1 = x[..., :half], x[..., half:]
    out[..., :half] = (x0 * cs).astype(F) - (x1 * sn).astype(F)
    out[..., half:] = (x1 * cs).astype(F) + (x0 * sn).astype(F)
    return out


def _rope(c: Case, ins: dict, F, mut):
    s, hq, hk, d = c.shape
    half = d // 2
    cs, sn = np.asarray(ins["cos"], F)[:, None, :half], np.asarray(ins["sin"], F)[:, None, :half]
    if mut == "sin_sign":
        sn = -sn
    if mut == "table_row_plus_one":
        cs, sn = np.roll(cs, -1, axis=0), np.roll(sn, -1, axis=0)
    adj = mut == "pairs_adjacent"
    q, k = np.asarray(ins["q"], F), np.asarray(ins["k"], F)
    out = {"q": _rotate(q, cs, sn, F, adj)}
    if mut == "k_heads_as_q_heads" and hk:
        pos = np.arange(s * hk) // hq                                # the position of a k row found with q's head count
        out["k"] = _rotate(k.reshape(s * hk, d), cs[pos, 0], sn[pos, 0], F).reshape(s, hk, d)
    else:
        out["k"] = _rotate(k, cs, sn, F, adj) if hk else k.copy()
    return out


# ---- what is expected -----------------------------------------------------------------------------------------------------------
def out_dtype(c: Case, name: str) -> str:
    return operands(c)[name][0]


def is_exact(c: Case) -> bool:
    if c.fam == "binary":
        return c.op != "div"
    if c.fam == "act":
        return c.op in ACT_EXACT
    if c.fam == "rope":
        return c.extra[1] == "exact"
    return c.fam in ("bias_add", "cast", "reduce", "sum_axis", "clamp", "where")


def bar_family(c: Case) -> str | None:
    """The key of MEASURED this case reports under (None: exact)."""
    if is_exact(c):
        return None
    if c.fam == "binary":
        return "div"
    if c.fam == "act":
        return c.op if c.op in ("sqrt", "rsqrt", "gelu") else "lib"
    if c.fam in ("glu", "glu_packed"):
        return "glu"
    return c.op if c.fam == "norm" else c.fam


def truncated(x, dt: str) -> np.ndarray:
    """The planted error of the casts: round toward zero."""
    x = np.ascontiguousarray(x, np.float32)
    if dt == "f32":
        return x.copy()
    if dt == "bf16":
        return ((x.view(np.uint32) >> 16) << 16).view(np.float32)
    with np.errstate(over="ignore"):
        h = x.astype(np.float16)
    h = np.where(np.isinf(h) & np.isfinite(x), np.copysign(np.float16(65504.0), h), h).astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(x)
    return np.where(over, np.nextafter(h, np.float16(0.0)), h).astype(np.float32)


@functools.lru_cache(maxsize=6)
def expected(c: Case) -> dict:
    """name -> ("words", words) or ("bar", v, bar) for every output: exact storage words, or the float64 value and the
    total bar (half an ulp of the output type included) that every element must stay inside."""
    ins = inputs(c)
    if is_exact(c):
        return {k: ("words", to_words(v, out_dtype(c, k))) for k, v in compute(c, ins, np.float32, sum_exact).items()}
    val = compute(c, ins, np.float64, sum_exact)
    f64 = lambda a: np.asarray(a, np.float64)      # noqa: E731
    bars = {}
    if c.fam == "binary":
        bars["c"] = 2 * U * np.abs(val["c"])
    elif c.fam == "act":
        bars["y"] = act_bar(c.op, val["y"])
        if c.op in EXACT_POINT and c.n >= NVEC[c.dtype]:
            assert val["y"].reshape(-1)[0] == EXACT_POINT[c.op][1]
            bars["y"].reshape(-1)[0] = 0.0
    elif c.fam in ("glu", "glu_packed"):
        if c.fam == "glu":
            act, g, up = ("silu" if c.op == "swiglu" else "gelu"), f64(ins["g"]), f64(ins["u"])
        else:
            act, g, up = c.op, f64(ins["gu"])[:, :c.shape[1]], f64(ins["gu"])[:, c.shape[1]:]
        bars["o"] = act_bar(act, act_fn(act, g, np.float64)) * np.abs(up) + U * np.abs(val["o"])
        bars["o"][g == 0.0] = 0.0                                 # silu(0) = gelu(0) = 0: the product is exactly 0
    elif c.fam == "softmax":
        x = f64(ins["x"])
        n = x.shape[1]
        m = x.max(axis=1, keepdims=True)
        with np.errstate(invalid="ignore"):
            e = np.exp(x - m)
            de = np.where(np.isneginf(x), 0.0, LIB_ATOL + (LIB_RTOL + U * np.abs(np.where(np.isneginf(x), 0.0, x - m))) * e)
        s = e.sum(axis=1, keepdims=True)
        bars["y"] = np.where(np.isneginf(x), 0.0, de / s + val["y"] * (de.sum(axis=1, keepdims=True) / s + (n + 2) * U))
    elif c.fam == "norm":
        bars["out"] = _norm_bar(c, ins, val["out"])
    else:
        assert c.fam == "rope", c.fam
        s, hq, hk, d = c.shape
        half = d // 2
        cs, sn = np.abs(f64(ins["cos"]))[:, None, :half], np.abs(f64(ins["sin"]))[:, None, :half]
        for name in ("q", "k"):
            x = np.abs(f64(ins[name]))
            x0, x1 = x[..., :half], x[..., half:]
            bars[name] = 2 * U * np.concatenate([x0 * cs + x1 * sn, x1 * cs + x0 * sn], axis=-1)
    return {k: ("bar", np.asarray(val[k], np.float64), total_bar(val[k], bars[k], out_dtype(c, k))) for k in val}


def _norm_bar(c: Case, ins: dict, v):
    n = c.shape[1]
    if c.op != "layernorm":
        return (n / 2 + (10 if c.op == "rmsnorm_residual" else 8)) * U * np.abs(v)
    x, g, b = (np.asarray(ins[k], np.float64) for k in ("x", "gamma", "beta"))
    mean = x.mean(axis=1, keepdims=True)
    dm = (n - 1) * U * np.abs(x).mean(axis=1, keepdims=True) + U * np.abs(mean)
    d = x - mean
    var = (d * d).mean(axis=1, keepdims=True)
    dvar = 2 * dm * np.abs(d).mean(axis=1, keepdims=True) + dm * dm + (n + 4) * U * var
    inv = 1.0 / np.sqrt(var + EPS)
    r = dvar / (2 * (var + EPS)) + 5 * U
    return np.abs(g)[None, :] * inv * (dm + U * np.abs(d)) + np.abs(d * inv * g[None, :]) * (r + 3 * U) + U * np.abs(v)


def initial_words(c: Case, name: str) -> np.ndarray:
    """What an output buffer holds before the call: the input for the in-place operands, the NaN guard pattern otherwise."""
    dt, shape, _ = operands(c)[name]
    if name in inputs(c):
        return to_words(inputs(c)[name], dt)
    return np.full(shape, GUARD_WORD[dt], np.uint16 if ITEM[dt] == 2 else np.uint32)


def emulate(c: Case, how: str, mut: str | None = None) -> dict:
    """name -> storage words of a float32 NumPy run of the case: how = "seq" (sums left to right), "pairwise" (a binary tree),
    or "f64" (float64 arithmetic rounded once, used for the planted errors)."""
    F, summ = {"seq": (np.float32, sum_seq), "pairwise": (np.float32, sum_pairwise), "f64": (np.float64, sum_exact)}[how]
    if is_exact(c):
        F = np.float32                       # the float32 operation, then one rounding
    ins = inputs(c)
    if mut == "truncate":
        return {"dst": canonical(to_words(truncated(ins["src"], c.extra[0]), c.extra[0]), c.extra[0])}
    out = compute(c, ins, F, summ, None if mut == "drop_tail" else mut)
    words = {}
    for k, v in out.items():
        dt = out_dtype(c, k)
        with np.errstate(over="ignore", invalid="ignore"):
            w = to_words(np.asarray(v, np.float64).astype(np.float32), dt)
        if mut == "drop_tail":                                    # the last n % N elements (or the last one) are never written
            keep = w.reshape(-1).copy()
            t = keep.size % NVEC[c.dtype] or 1
            keep[-t:] = initial_words(c, k).reshape(-1)[-t:]
            w = keep.reshape(w.shape)
        words[k] = w
    return words


def mutations(c: Case) -> tuple:
    """The planted errors that apply to the case; each must put at least one element outside its bar (or change a word)."""
    n = c.n
    if c.fam in ("binary", "act", "glu", "glu_packed", "clamp", "where"):
        return ("drop_tail",) + (("shift_one",) if n > 1 else ())
    if c.fam == "bias_add":
        return ("drop_tail", "shift_one") + (("neighbour_column",) if c.shape[1] > 1 else ())
    if c.fam == "cast":
        narrowing = ITEM[c.extra[0]] < ITEM[c.dtype] or (c.dtype, c.extra[0]) in (("bf16", "f16"), ("f16", "bf16"))
        return ("drop_tail",) + (("shift_one",) if n > 1 else ()) + (("truncate",) if narrowing and n >= 1027 else ())
    if c.fam == "norm":
        rows, f = c.shape
        m = ["drop_tail", "no_eps"]
        if f > 1:
            m += ["shift_one", "neighbour_column"]
        if rows > 1:
            m.append("previous_row_statistic")
        if c.op == "rmsnorm_residual":
            m.append("no_residual")
        if c.op == "layernorm" and f > 1 and rows > 2:                # needs the row with mean 100
            m.append("variance_without_mean")
        return tuple(m)
    if c.fam == "rope":
        s, hq, hk, d = c.shape
        m = ["sin_sign", "table_row_plus_one"]
        if d > 2:
            m.append("pairs_adjacent")
        if hk and hq != hk:
            m.append("k_heads_as_q_heads")
        return tuple(m)
    if c.fam == "reduce":
        if c.op in ("max", "min"):
            return ("ignore_last",) if c.extra[0] == n - 1 and n > 1 else ()
        m = ["ignore_last"] if n > 1 else []
        if c.op == "mean" and n > 1 and (c.dtype == "f32" or 1.0 / n >= 4 * HALF_ULP[c.dtype]):
            m.append("mean_n_minus_1")
        return tuple(m)
    if c.fam == "softmax":
        return (("drop_last",) if c.shape[1] > 1 else ()) + (("no_max_subtraction",) if c.shape[0] > 1 else ())
    assert c.fam == "sum_axis", c.fam
    return ("drop_last",) if (c.shape[1] if c.op == "axis1" else c.shape[0]) > 1 else ()


def mismatches(c: Case, got: dict) -> dict:
    """name -> boolean mask of the elements of `got` (storage words per output) that miss what expected(c) allows."""
    bad = {}
    for k, e in expected(c).items():
        dt = out_dtype(c, k)
        w = np.asarray(got[k])
        if w.shape != e[1].shape:
            bad[k] = np.ones(e[1].shape, bool)
        elif e[0] == "words":
            bad[k] = canonical(w, dt) != e[1]
        else:
            g = from_words(w, dt).astype(np.float64)
            with np.errstate(invalid="ignore"):
                bad[k] = ~(np.abs(g - e[1]) <= e[2])
    return bad


def used(c: Case, got: dict) -> float:
    """Largest fraction of its bar that an element of `got` uses (bar cases only)."""
    worst = 0.0
    for k, e in expected(c).items():
        if e[0] != "bar":
            continue
        g = from_words(np.asarray(got[k]), out_dtype(c, k)).astype(np.float64)
        err = np.abs(g - e[1])
        with np.errstate(divide="ignore", invalid="ignore"):
            frac = np.where(e[2] > 0, err / e[2], np.where(err == 0, 0.0, np.inf))
        worst = max(worst, float(np.nan_to_num(frac, nan=np.inf).max()) if frac.size else 0.0)
    return worst


def explain(c: Case, got: dict, limit: int = 6) -> str:
    """The first few mismatching elements of every output, for an assertion message."""
    lines = []
    for k, mask in mismatches(c, got).items():
        idx = np.argwhere(mask)
        if not idx.size:
            continue
        e = expected(c)[k]
        dt = out_dtype(c, k)
        g = from_words(np.asarray(got[k]), dt) if np.asarray(got[k]).shape == e[1].shape else None
        lines.append(f"{c}: output {k}: {idx.shape[0]} of {mask.size} elements differ")
        for i in map(tuple, idx[:limit]):
            if g is None:
                break
            if e[0] == "words":
                lines.append(f"  {i}: got {g[i]!r} (0x{int(np.asarray(got[k])[i]):x}), expected {from_words(e[1], dt)[i]!r} (0x{int(e[1][i]):x})")
            else:
                lines.append(f"  {i}: got {g[i]!r}, expected {e[1][i]!r} +- {e[2][i]:.3e} (off by {abs(float(g[i]) - e[1][i]):.3e})")
    return "\n".join(lines)
