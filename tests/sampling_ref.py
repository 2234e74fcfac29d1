"""Construction of the exact sampling tests (tests/test_sampling_exact_cpu.py proves it, tests/test_sampling_exact_gpu.py runs it).

The sampler (csrc/ops_sampling.hip, restated by oracle.cpu_ref.sample_token_u) is a function of (logits, T, top_k, top_p, u).
A random u on a random row checks the draw and hardly the KEPT SET: one token more or less, a wrong tie-break or a lost
slice moves every boundary by less than any margin a float comparison needs.  Two facts make the kept set readable:

  * exact masses: mass = floor(exp(z - max z) * 2^32) is exactly 2^32 at the row maximum and exactly 0 from 23 below it
    (exp(-23) * 2^32 < 1) and at -inf.  A PLATEAU ROW - a set P of indices at one value, every other token at least 30
    below it after the division by T - has the same integer masses on the device and in the oracle, bit for bit;
  * the draw walks the kept tokens in ascending index order, so with n mass-carrying kept tokens
    u_j = float32((j + 0.5) / n) returns exactly the j-th of them: walking j reads the kept set out of the kernel.
    u = j / n (n a power of two) sits exactly ON a boundary and returns token j - 1: that pins `>=` in the draw, as
    top_p = 0.5 / 0.75 on 4 / 8 / 1024 equal tokens pins `>=` and the ceiling in the nucleus cut.

Every product the kernels form from these numbers is exact in double (u: 24 bits, n * 2^32: at most 17 significant bits),
so the expected token is a closed form (kept_sets / expected_token below) and needs no margin.  Only the GRADED rows
(three or four value levels within 6 of the maximum, masses inexact on the device) use one: u is taken at the midpoint
of tokens whose own interval is at least 1e-3 of the kept mass, so every draw is 5e-4 from a boundary - above the 1e-4
the suite already allows expf against np.exp.

`restated` is a small mutable copy of the sampler; its mutants are the errors the case table must reject.
"""

from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

SLICE = 4096          # tokens per stage-1 workgroup            (SMP_SLICE)
MAX_K = 1024          # largest top_k of the sliced shape         (SMP_MAX_K)
WHOLE_K = 256         # candidates of the whole-vocabulary nucleus (SMP_WHOLE_K)
ONE = 1 << 32         # integer mass of a token at the row maximum
DTYPES = ("f32", "f16", "bf16")


def launch_shape(k: int, V: int, p: float) -> str:
    """The launch sequence sample_launch picks when it has a scratch buffer."""
    if 1 <= k <= MAX_K and k < V:
        return "sliced"
    if k == 0 and V > 2 * SLICE:
        return "vocab_nucleus" if p < 1.0 else "vocab_multinomial"
    return "whole_row"


def per_wave(V: int) -> int:
    """Tokens each of the 16 waves owns in the whole-row kernel's draw."""
    return ((V + 15) // 16 + 63) & ~63


# ---- plateau rows --------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Row:
    V: int
    spans: tuple = ()          # half-open index ranges of the plateau; () = the whole row
    value: float = 1.0         # representable in f32, f16 and bf16
    low: float = -120.0        # every other token (-inf allowed)
    zeros: bool = False        # the plateau is 0.0 with both signs mixed (value must be 0.0)
    lead: float | None = None  # the plateau's first index holds this value instead: fl(lead / T) == fl(value / T)

    def plateau(self) -> np.ndarray:
        if not self.spans:
            return np.arange(self.V, dtype=np.int64)
        return np.concatenate([np.arange(a, b, dtype=np.int64) for a, b in self.spans])


def negative_zero(idx: np.ndarray) -> np.ndarray:
    """Which plateau indices of a `zeros` row hold -0.0: a fixed scramble of the index, about half of them."""
    return ((idx * 2654435761) >> 13) & 1 == 1


@functools.lru_cache(maxsize=16)
def build_row(row: Row) -> np.ndarray:
    x = np.full(row.V, row.low, np.float32)
    P = row.plateau()
    x[P] = np.float32(row.value)
    if row.zeros:
        x[P] = np.where(negative_zero(P), np.float32(-0.0), np.float32(0.0))
    if row.lead is not None:
        x[P[0]] = np.float32(row.lead)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=64)
def kept_sets(row: Row, k: int, p: float):
    """(K, Z): the kept indices that carry mass 2^32 and the kept indices that carry none, both ascending - the contract
    (top-k by z with ties lowest index first, then the nucleus inside what top-k kept) in closed form."""
    P, V = row.plateau(), row.V
    Z = np.empty(0, np.int64)
    if 0 < k < V and k <= P.size:
        K = P[:k]
    else:
        K = P
        rest = np.setdiff1d(np.arange(V, dtype=np.int64), P)
        Z = rest[:k - P.size] if 0 < k < V else rest
    if p < 1.0:
        target = max(math.ceil(Fraction(float(np.float32(p))) * (int(K.size) * ONE)), 1)
        K, Z = K[:-(-target // ONE)], np.empty(0, np.int64)
    return K, Z


def expected_token(K: np.ndarray, Z: np.ndarray, u: float) -> int:
    """The first kept token, ascending index, whose inclusive mass reaches u * (kept mass); u = 0 is reached by the lowest
    kept index even when its mass is 0 (the oracle's definition), u = 1 by the highest kept index that has mass."""
    thr = Fraction(float(np.float32(u))) * (int(K.size) * ONE)
    if thr == 0:
        return int(min(K[0], Z[0])) if Z.size else int(K[0])
    return int(K[min(math.ceil(thr / ONE) - 1, K.size - 1)])


def pick_js(K: np.ndarray, V: int, seed: int, fill: int = 20) -> list[int]:
    """Positions in the kept set to draw: first, last, the neighbours of every 4096-token slice edge and of every per-wave
    partition edge of the whole-row draw that falls inside the kept set, and a seeded random remainder."""
    n = int(K.size)
    js = {0, n - 1}
    for e in sorted(set(range(SLICE, V, SLICE)) | set(range(per_wave(V), V, per_wave(V)))):
        pos = int(np.searchsorted(K, e))
        if 0 < pos < n:
            js |= {pos - 1, pos}
    rng = np.random.default_rng(seed)
    while len(js) < min(max(fill, len(js)), n):
        js.add(int(rng.integers(0, n)))
    return sorted(js)


@dataclass(frozen=True)
class Case:
    name: str
    rows: tuple                # Rows of one V: one launch
    k: int
    p: float = 1.0
    T: float = 1.0
    dtypes: tuple = ("f32",)

    @property
    def V(self) -> int:
        return self.rows[0].V

    @property
    def shape(self) -> str:
        return launch_shape(self.k, self.V, self.p)

    def __str__(self) -> str:
        return self.name


def case_us(case: Case) -> list[float]:
    """The u of a case's launches.  Every row of the launch is checked at every u (expected_token holds for any u), so
    the midpoints and boundaries of one row are off-centre draws of the others."""
    us = {0.0, 1.0}
    for r, row in enumerate(case.rows):
        K, _ = kept_sets(row, case.k, case.p)
        n = int(K.size)
        js = pick_js(K, row.V, seed=len(case.name) * 131 + r)
        us |= {float(np.float32((j + 0.5) / n)) for j in js}
        if n & (n - 1) == 0:                                    # exactly on a boundary: j / n is a float32
            us |= {float(np.float32(j / n)) for j in js[:6] + js[-6:]}
    return sorted(us)


def _ragged(V: int) -> tuple:
    """A plateau wholly inside the last, ragged slice that includes index V - 1."""
    lo = (V - 1) // SLICE * SLICE
    return ((max(lo, V - 40), V),)


def find_pair(T: float, seed: int = 5) -> tuple[float, float]:
    """Adjacent floats a < b that the division by T maps to one float and a multiplication by fl(1 / T) does not."""
    rng = np.random.default_rng(seed)
    t = np.float32(T)
    a = rng.uniform(1.0, 8.0, 1 << 14).astype(np.float32)
    b = np.nextafter(a, np.float32(np.inf))
    r = np.float32(1.0) / t
    hit = np.nonzero((a / t == b / t) & (a * r != b * r))[0]
    return float(a[hit[0]]), float(b[hit[0]])


def _cases() -> dict:
    g: dict[str, list[Case]] = {f"g{i}": [] for i in range(1, 8)}
    A = DTYPES

    # 1. launch shapes by (k, V)
    for V in (4095, 4096, 4097, 8193):
        for p in (1.0, 0.5):
            g["g1"].append(Case(f"g1_sliced_equal_V{V}_p{p}", (Row(V), Row(V, _ragged(V))), 50, p, dtypes=A))
    g["g1"] += [
        Case("g1_sliced_last_slice_of_one_V4097", (Row(4097, ((4096, 4097),)), Row(4097, ((4095, 4097),), low=-np.inf)), 50, dtypes=A),
        Case("g1_sliced_last_slice_of_one_V8193", (Row(8193, ((8192, 8193),)), Row(8193, ((4095, 4097), (8191, 8193)))), 3, dtypes=A),
        Case("g1_sliced_ragged_plateau_V4200_k50", (Row(4200, ((4100, 4200),)),), 50, dtypes=A),
        Case("g1_sliced_ragged_plateau_V4200_k50_p0.5", (Row(4200, ((4100, 4200),)),), 50, 0.5, dtypes=A),
        Case("g1_sliced_ragged_plateau_V4200_k128", (Row(4200, ((4100, 4200),)),), 128, dtypes=A),
        Case("g1_sliced_across_edges_V8193_k230", (Row(8193, ((4000, 4200), (8150, 8193))),), 230, dtypes=A),
        Case("g1_sliced_across_edges_V8193_k243", (Row(8193, ((4000, 4200), (8150, 8193))),), 243, dtypes=A),
        Case("g1_whole_k1025_V4097", (Row(4097), Row(4097, ((3000, 4097),))), 1025, dtypes=A),
        Case("g1_whole_k1025_V4097_p0.5", (Row(4097), Row(4097, ((3000, 4097),))), 1025, 0.5, dtypes=A),
        Case("g1_whole_k1025_ragged_V4200", (Row(4200, ((3000, 4200),)),), 1025, dtypes=A),
        Case("g1_whole_k_eq_V1025", (Row(1025), Row(1025, _ragged(1025))), 1025, dtypes=A),
        Case("g1_whole_k_gt_V1025", (Row(1025), Row(1025, _ragged(1025))), 5000, 0.5, dtypes=A),
    ]
    for V in (7, 63, 64, 65, 1023, 1024, 1025):
        rows = (Row(V), Row(V, ((V - 3, V),)))
        g["g1"] += [Case(f"g1_whole_tiny_V{V}", rows, 0, dtypes=A), Case(f"g1_whole_tiny_V{V}_p0.5", rows, 0, 0.5, dtypes=A),
                    Case(f"g1_sliced_tiny_V{V}_k3", rows, 3, dtypes=A)]
    for V in (8193, 12325):
        rows = (Row(V), Row(V, _ragged(V)), Row(V, ((4090, 4100),), low=-np.inf))
        g["g1"] += [Case(f"g1_vocab_multinomial_V{V}", rows, 0, dtypes=A), Case(f"g1_vocab_nucleus_V{V}_p0.5", rows, 0, 0.5, dtypes=A)]

    # 2. k at the stage-2 sort switch (rank sort up to 128 keys, bitonic above), p = 1 and a p that cuts inside
    for k in (1, 2, 127, 128, 129, 1023, 1024):
        for p in (1.0, 0.5):
            g["g2"].append(Case(f"g2_k{k}_p{p}", (Row(4097), Row(4097, ((3000, 4097),))), k, p, dtypes=A))

    # 3. the nucleus is cut within what top-k kept, not within the row
    g["g3"] += [Case("g3_nucleus_within_topk_sliced", (Row(100),), 10, 0.5), Case("g3_nucleus_within_topk_whole", (Row(3000),), 1100, 0.5)]

    # 4. the whole-vocabulary decision: n <= 256 ends in the candidate kernel, n >= 257 falls through; the ragged rows
    #    of the same launch always end in the candidate kernel
    for V in (8193, 12325):
        for n in (255, 256, 257, 300):
            g["g4"].append(Case(f"g4_decision_V{V}_n{n}", (Row(V), Row(V, _ragged(V))), 0, float(np.float32((n - 0.5) / V))))

    # 5. ties across index bytes (65535 | 65536 and 255 | 256): the low-word radix passes
    g["g5"] += [
        Case("g5_index_bytes_sliced_k700", (Row(65536 + 700, ((65000, 66000),)),), 700),
        Case("g5_index_bytes_sliced_k700_p0.9", (Row(65536 + 700, ((65000, 66000),)),), 700, 0.9),
        Case("g5_index_bytes_whole_k1025", (Row(65536 + 1100, ((65000, 66500),)),), 1025),
        Case("g5_index_bytes_whole_k1025_p0.75", (Row(65536 + 1100, ((65000, 66500),)),), 1025, 0.75),
        Case("g5_index_bytes_vocab_nucleus_p0.5", (Row(65536 + 1100, ((65000, 66500),)),), 0, 0.5),
        Case("g5_index_255_256_k80", (Row(4096, ((200, 300),)),), 80),
    ]

    # 6. signed zeros: kept by index alone
    zs = dict(value=0.0, zeros=True)
    g["g6"] += [
        Case("g6_zeros_sliced_k20", (Row(4097, ((10, 60), (4090, 4097)), **zs),), 20, dtypes=A),
        Case("g6_zeros_sliced_k40_p0.5", (Row(4097, ((10, 60), (4090, 4097)), **zs),), 40, 0.5, dtypes=A),
        Case("g6_zeros_sliced_k57_p0.5", (Row(4097, ((10, 60), (4090, 4097)), **zs),), 57, 0.5, dtypes=A),
        Case("g6_zeros_whole_k1025", (Row(4097, ((0, 1500),), **zs),), 1025, dtypes=A),
        Case("g6_zeros_whole_k1025_p0.5", (Row(4097, ((0, 1500),), **zs),), 1025, 0.5, dtypes=A),
        Case("g6_zeros_whole_tiny_p0.5", (Row(65, **zs),), 0, 0.5, dtypes=A),
        Case("g6_zeros_vocab_nucleus_p0.25", (Row(8193, ((0, 600),), **zs),), 0, 0.25, dtypes=A),
        Case("g6_zeros_vocab_nucleus_p0.5", (Row(8193, ((0, 600),), **zs),), 0, 0.5, dtypes=A),
    ]

    # 7. temperature is a division: `lead` (a) sits at the lowest plateau index and ties with b only under a true division
    for T in (3.0, 0.7, 1.3):
        a, b = find_pair(T)
        pr = dict(value=b, lead=a, low=-300.0)
        g["g7"] += [
            Case(f"g7_T{T}_k1_sliced", (Row(4097, ((4000, 4002),), **pr),), 1, T=T),
            Case(f"g7_T{T}_kth_sliced", (Row(4097, ((4046, 4097),), **pr),), 50, T=T),
            Case(f"g7_T{T}_kth_whole", (Row(4097, ((100, 1126),), **pr),), 1025, T=T),
            Case(f"g7_T{T}_nucleus_whole_tiny", (Row(65, ((61, 65),), **pr),), 0, 0.75, T=T),
            Case(f"g7_T{T}_nucleus_vocab", (Row(8193, ((8189, 8193),), **pr),), 0, 0.75, T=T),
        ]
    # cases of groups 1, 2 and 6 again at a temperature that is no power of two, in every dtype (the plateau stays the maximum)
    more = ("g1_whole_k1025_V4097_p0.5", "g1_whole_tiny_V65_p0.5", "g1_vocab_multinomial_V12325", "g1_vocab_nucleus_V12325_p0.5",
            "g6_zeros_whole_k1025_p0.5", "g6_zeros_vocab_nucleus_p0.5")
    again = g["g1"][:8] + g["g2"][6:10] + g["g6"][:2] + [c for c in g["g1"] + g["g6"] if c.name in more]
    g["g7"] += [Case(c.name + "_T0.7", c.rows, c.k, c.p, 0.7, c.dtypes) for c in again]
    return g


GROUPS = _cases()
CASES = [c for grp in GROUPS.values() for c in grp]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---- graded rows ---------------------------------------------------------------------------------------------------------

LEVELS = (0.0, -1.25, -2.5, -5.5)
MIN_SHARE, GRADED_MARGIN = 1e-3, 5e-4


@dataclass(frozen=True)
class Graded:
    name: str
    V: int
    k: int
    p: float = 1.0
    T: float = 1.0
    live: int = 60             # random tokens on a level (plus both ends and the slice edges); every other token is 120 below
    data: tuple = ()           # an explicit row instead

    @property
    def shape(self) -> str:
        return launch_shape(self.k, self.V, self.p)

    def __str__(self) -> str:
        return self.name


@functools.lru_cache(maxsize=8)
def build_graded(c: Graded) -> np.ndarray:
    if c.data:
        return np.asarray(c.data, np.float32)
    rng = np.random.default_rng(c.V * 7 + c.live)
    edges = [e + d for e in range(SLICE, c.V, SLICE) for d in (-1, 0)]
    idx = np.unique(np.concatenate([[0, c.V - 1], edges, rng.choice(c.V, min(c.live, c.V), replace=False)]).astype(np.int64))
    x = np.full(c.V, -120.0, np.float32)
    x[idx] = np.asarray(LEVELS, np.float32)[rng.integers(0, len(LEVELS), idx.size)]
    x[idx[0]] = 0.0                                                                 # the maximum is on the grid
    return x


def graded_us(c: Graded, limit: int = 48) -> list[float]:
    """Midpoints of the kept tokens whose own interval is at least MIN_SHARE of the kept mass."""
    idx, cum = prepare(build_graded(c), c.T, c.k, c.p)
    q = np.diff(cum, prepend=0.0)
    heavy = np.nonzero(q >= MIN_SHARE * cum[-1])[0]
    if heavy.size > limit:
        rng = np.random.default_rng(len(c.name))
        heavy = np.unique(np.concatenate([heavy[:2], heavy[-2:], rng.choice(heavy, limit - 4, replace=False)]))
    return [float(np.float32((cum[j] - q[j] / 2) / cum[-1])) for j in heavy]


GRADED = [
    Graded("g9_sliced_V4095_k40", 4095, 40), Graded("g9_sliced_V4096_k40_p0.9", 4096, 40, 0.9),
    Graded("g9_sliced_V4097_k40_T0.8", 4097, 40, 1.0, 0.8), Graded("g9_sliced_V8193_k40_p0.9_T1.3", 8193, 40, 0.9, 1.3),
    Graded("g9_sliced_V8193_k200", 8193, 200, live=300),
    Graded("g9_whole_k1025_V4097", 4097, 1025), Graded("g9_whole_k1025_V4097_p0.9", 4097, 1025, 0.9, live=300),
    Graded("g9_whole_tiny_V65", 65, 0, live=40), Graded("g9_whole_tiny_V1023_p0.9", 1023, 0, 0.9),
    Graded("g9_vocab_multinomial_V8193", 8193, 0), Graded("g9_vocab_multinomial_V12325_T0.8", 12325, 0, 1.0, 0.8, live=200),
    Graded("g9_vocab_nucleus_candidates_V8193_p0.9", 8193, 0, 0.9), Graded("g9_vocab_nucleus_candidates_V12325_p0.9", 12325, 0, 0.9),
    Graded("g9_vocab_nucleus_falls_through_V8193_p0.99", 8193, 0, 0.99, live=400),
    Graded("g9_vocab_nucleus_falls_through_V12325_p0.99", 12325, 0, 0.99, live=400),
    # the signed-zero example of the contract: top-2 of [1, -0, +0, -3, +0, -0] is {0, 1}
    Graded("g9_signed_zero_example_k2", 6, 2, data=(1.0, -0.0, 0.0, -3.0, 0.0, -0.0)),
    Graded("g9_signed_zero_example_k3_p0.9", 6, 3, 0.9, data=(1.0, -0.0, 0.0, -3.0, 0.0, -0.0)),
]


# ---- a mutable restatement of the sampler ----------------------------------------------------------------------------------

MUTANTS = ("topk_minus_1", "topk_plus_1", "ties_highest_index", "signed_zero_key", "recip_temperature", "nucleus_gt",
           "nucleus_whole_row_mass", "draw_gt", "draw_descending_z", "slices_not_merged", "ragged_slice_dropped", "vocab_nucleus_cut_256")


def prepare(logits: np.ndarray, T: float, k: int, p: float, mut: str = ""):
    """(kept indices in draw order, their inclusive cumulative integer masses as float64)."""
    x = np.asarray(logits, np.float32)
    t = np.float32(T)
    z = (x * (np.float32(1.0) / t) if mut == "recip_temperature" else x / t).astype(np.float32)
    V = z.size
    shape = launch_shape(k, V, p)
    alive = np.ones(V, bool)
    if mut == "ragged_slice_dropped" and shape != "whole_row" and V > SLICE and V % SLICE:
        alive[V // SLICE * SLICE:] = False
        z[~alive] = -np.inf
    q = np.floor(np.exp(z - z[alive].max()).astype(np.float32).astype(np.float64) * 4294967296.0)
    zk = z.astype(np.float64)
    if mut == "signed_zero_key":
        zk = np.where((z == 0) & np.signbit(z), -1e-300, zk)
    tie = -np.arange(V) if mut == "ties_highest_index" else np.arange(V)
    order = np.lexsort((tie, -zk))
    order = order[alive[order]]
    kept = alive.copy()
    if 0 < k < V:
        kk = max(k - 1, 1) if mut == "topk_minus_1" else k + 1 if mut == "topk_plus_1" else k
        kept[:] = False
        if mut == "slices_not_merged" and shape == "sliced":
            for lo in range(0, V, SLICE):
                o = order[(order >= lo) & (order < lo + SLICE)]
                kept[o[:kk]] = True
        else:
            kept[order[:kk]] = True
    if p < 1.0:
        o = order[kept[order]]
        if mut == "vocab_nucleus_cut_256" and shape == "vocab_nucleus":
            total, o = q[o].sum(), o[:WHOLE_K]
        else:
            total = q[alive].sum() if mut == "nucleus_whole_row_mass" else q[o].sum()
        cum = np.cumsum(q[o])
        target = max(float(np.ceil(np.float64(np.float32(p)) * total)), 1.0)
        n = min(int(np.searchsorted(cum, target, side="right" if mut == "nucleus_gt" else "left")) + 1, o.size)
        kept[:] = False
        kept[o[:n]] = True
    idx = order[kept[order]] if mut == "draw_descending_z" else np.nonzero(kept)[0]
    return idx, np.cumsum(q[idx])


def draw(prep, u: float, mut: str = "") -> int:
    idx, cum = prep
    thr = np.float64(np.float32(u)) * cum[-1]
    pos = int(np.searchsorted(cum, thr, side="right" if mut == "draw_gt" else "left"))
    return int(idx[min(pos, idx.size - 1)])


def restated(logits: np.ndarray, T: float, k: int, p: float, u: float, mut: str = "") -> int:
    return draw(prepare(logits, T, k, p, mut), u, mut)


def rejects(case, mut: str) -> bool:
    """Does the case's expectation differ from what the mutated sampler returns, for some row and u?"""
    if isinstance(case, Graded):
        row = build_graded(case)
        good, bad = prepare(row, case.T, case.k, case.p), prepare(row, case.T, case.k, case.p, mut)
        return any(draw(good, u) != draw(bad, u, mut) for u in graded_us(case))
    us = case_us(case)
    for row in case.rows:
        K, Z = kept_sets(row, case.k, case.p)
        bad = prepare(build_row(row), case.T, case.k, case.p, mut)
        if any(expected_token(K, Z, u) != draw(bad, u, mut) for u in us):
            return True
    return False


# the case that is named for each mutant (tests/test_sampling_exact_cpu.py asserts each pair)
REJECTED_BY = {
    "topk_minus_1": "g2_k128_p1.0", "topk_plus_1": "g2_k128_p1.0", "ties_highest_index": "g5_index_bytes_sliced_k700",
    "signed_zero_key": "g6_zeros_sliced_k20", "recip_temperature": "g7_T3.0_k1_sliced", "nucleus_gt": "g2_k128_p0.5",
    "nucleus_whole_row_mass": "g3_nucleus_within_topk_sliced", "draw_gt": "g2_k128_p1.0", "draw_descending_z": "g9_sliced_V4095_k40",
    "slices_not_merged": "g1_sliced_equal_V4097_p1.0", "ragged_slice_dropped": "g1_sliced_ragged_plateau_V4200_k50",
    "vocab_nucleus_cut_256": "g4_decision_V8193_n257",
}


# ---- host <-> device -------------------------------------------------------------------------------------------------------

def rounded(x: np.ndarray, dtype: str) -> np.ndarray:
    """The float32 value the device holds for x in `dtype`."""
    from oracle import cpu_ref as O

    x = np.asarray(x, np.float32)
    return x if dtype == "f32" else x.astype(np.float16).astype(np.float32) if dtype == "f16" else O.bf16_round(x)
