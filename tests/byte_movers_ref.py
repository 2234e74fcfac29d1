"""Cases, oracle and planted errors of the byte movers: the layout shuffles, gathers, KV-cache writes and argmax of
csrc/ops_tensor.hip, the paged-cache write and the continuous-batching helpers of csrc/ops_paged.hip, through every public
entry point (ops/tensor.py, ops/embedding.py, ops/paged.py, ops/reduction.py, ops/nn/linear.py, ops.transpose,
GPUArray.transpose / reshape).  Used by tests/test_byte_movers_cpu.py (no device) and tests/test_byte_movers_gpu.py.

Every case names the family and the entry point, the item type, the shape, the operands that sit off 16-byte alignment and by
how many elements, the leaf ops.tensor_op_plan must report (None where the path has one kernel and no width choice, or is a
device-to-device copy) and whether the grid-stride loop takes a second trip.  Inputs are storage words from a seeded generator,
never equal to the canary word; the oracle is NumPy's own indexing on those words (swapaxes, repeat, take, slices and fancy
assignment), not the kernels' index arithmetic.  These ops are exact: outputs are compared word for word.

argmax follows the kernels' rule, which is not np.argmax's: NaN is skipped, the largest remaining value wins, ties go to the
lowest index (+0.0 and -0.0 tie), and a row with no value above -inf gives 0.

The planted errors (PLANTED) corrupt the oracle's output the way a slip in a kernel would; the CPU test shows that each one
changes at least one word of every case it applies to, so the comparison on the device would notice."""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

BLOCK = 256
CAP = 4096                       # blocks; a grid-stride mover wraps beyond CAP * BLOCK work items
WORD = {"u8": np.uint8, "bf16": np.uint16, "f16": np.uint16, "f32": np.uint32, "i64": np.uint64, "i32": np.int32}
ITEM = {"u8": 1, "bf16": 2, "f16": 2, "f32": 4, "i64": 8, "i32": 4}
DTYPE_NAME = {"u8": "uint8", "bf16": "bfloat16", "f16": "float16", "f32": "float32", "i64": "int64", "i32": "int32"}
CANARY = {"u8": 0xC5, "bf16": 0xFFC5, "f16": 0xFFC5, "f32": 0xFFC5C5C5, "i64": 0xC5C5C5C5C5C5C5C5, "i32": -0x3A3A3A3B}   # NaN words for the floats
VEC_LEAVES = ("vec16", "vec8", "vec4", "vec2", "vec1")
PLANTED = ("swap_in_ragged_tile", "row_off_by_one", "wrong_width_stride", "drop_last_vector", "drop_second_trip", "head_mod_for_div",
           "tile_for_repeat", "position_plus_one", "k_v_exchanged", "slot_div_mod_exchanged", "start_plus_len", "inclusive_sum",
           "highest_index_on_ties", "first_wave_only", "nan_wins")


@dataclass(frozen=True)
class Case:
    fam: str                     # transpose, row_map, split_qkv, gather, slice, kv_write, seq_copy, argmax, paged_write, scatter_last, position_ids, check_eos, cumsum, batch_inputs
    entry: str                   # the public entry point
    item: str
    shape: tuple
    mis: tuple = ()              # ((operand, elements off alignment), ...)
    leaf: str | None = None
    wrap: bool = False
    extra: tuple = ()

    def __str__(self):
        return f"{self.fam}/{self.entry}/{self.item}/{'x'.join(map(str, self.shape))}" + (f"/mis={dict(self.mis)}" if self.mis else "") + \
            (f"/{self.extra}" if self.extra else "") + ("/wrap" if self.wrap else "")


@dataclass
class Op:
    """One operand: its words, and its role - "in", "out" (given by the caller, pre-filled with the canary), "inout" (a cache:
    given by the caller, holds words before the call) or "ret" (allocated by the wrapper and returned)."""
    item: str
    words: np.ndarray
    role: str
    guard: int = 0               # guard elements on each side beyond the 16 bytes every operand gets


def _seed(c: Case) -> int:
    return int.from_bytes(str(c).encode(), "little") % (2 ** 32)


def words(rng, item: str, shape) -> np.ndarray:
    """Random storage words, none equal to the canary."""
    bits = 8 * ITEM[item]
    w = rng.integers(0, 2 ** bits, size=shape, dtype=np.uint64, endpoint=False).astype(WORD[item]) if bits < 64 else \
        rng.integers(0, 2 ** 63, size=shape, dtype=np.uint64)
    w = np.asarray(w, WORD[item])
    w[w == WORD[item](CANARY[item])] ^= WORD[item](1)
    return w


def canary(item: str, shape) -> np.ndarray:
    return np.full(shape, CANARY[item], WORD[item])


def i32(v) -> np.ndarray:
    return np.atleast_1d(np.asarray(v, np.int32))


# ---- float rows for argmax -------------------------------------------------------------------------------------------------------
def float_words(x: np.ndarray, item: str) -> np.ndarray:
    """Words of float32 values that the item type holds exactly (the argmax rows use small integers, 0, inf and NaN only)."""
    x = np.asarray(x, np.float32)
    if item == "f32":
        return x.view(np.uint32).copy()
    if item == "f16":
        h = x.astype(np.float16)
        assert ((h.astype(np.float32) == x) | np.isnan(x)).all()
        return h.view(np.uint16).copy()
    u = x.view(np.uint32)
    assert ((u & 0xFFFF) == 0).all()
    return (u >> 16).astype(np.uint16)


def words_float(w: np.ndarray, item: str) -> np.ndarray:
    if item == "f32":
        return np.asarray(w, np.uint32).view(np.float32)
    if item == "f16":
        return np.asarray(w, np.uint16).view(np.float16).astype(np.float32)
    return (np.asarray(w, np.uint16).astype(np.uint32) << 16).view(np.float32)


def argmax_rule(row: np.ndarray, ties: str = "lowest", nan_wins: bool = False, keep=None) -> int:
    """The kernels' rule on one float32 row (module docstring).  `keep`: a mask of the elements that take part."""
    row = np.asarray(row, np.float32)
    idx = np.arange(row.size)
    if keep is not None:
        row, idx = row[keep], idx[keep]
    if nan_wins and np.isnan(row).any():
        return int(idx[np.flatnonzero(np.isnan(row))[0]])
    ok = ~np.isnan(row) & (row > -np.inf)
    if not ok.any():
        return 0
    best = row[ok].max()
    at = idx[ok & (row == best)]
    return int(at[0] if ties == "lowest" else at[-1])


ARGMAX_N = (1, 63, 64, 65, 255, 256, 257, 16383, 16384, 16385, 151936)
ARGMAX_KINDS = ("single", "wave1", "tie_stride", "tie_lanes", "tie_waves", "tie_ends", "neg_inf", "pos_inf_tie", "zeros", "nan", "all_nan")


def argmax_block(n: int) -> int:
    """Threads per row, as the leaf of the case says (block256 / block1024)."""
    return 1024 if n >= 16384 else 256


def argmax_places(kind: str, n: int):
    """Indices where the maximum is planted, or None when the row is too short for the kind."""
    B = argmax_block(n)
    places = {"single": (n // 3,), "wave1": (64 + (n - 65) % 192,) if n > 64 else None, "tie_stride": (5, 5 + B) if n > 5 + B else None,
              "tie_lanes": (3, 40) if n > 40 else None, "tie_waves": (71, 130) if n > 130 else None, "tie_ends": (0, n - 1) if n >= 2 else None,
              "neg_inf": (), "pos_inf_tie": (n // 2, n - 2) if n >= 4 else None, "zeros": (n // 4, n - 1) if n >= 8 else None,
              "nan": (n // 2,) if n >= 4 else None, "all_nan": ()}
    return places[kind]


def argmax_row(rng, kind: str, n: int) -> np.ndarray:
    at = argmax_places(kind, n)
    x = rng.integers(-100, 101, size=n).astype(np.float32)
    if kind == "neg_inf":
        x[:] = -np.inf
    elif kind == "all_nan":
        x[:] = np.nan
    elif kind == "pos_inf_tie":
        x[list(at)] = np.inf
    elif kind == "zeros":                 # -0.0 first, +0.0 later, everything else negative: equal, the lowest index wins
        x = -np.abs(x) - 1
        x[at[0]], x[at[1]] = -0.0, 0.0
    elif kind == "nan":                   # NaN at the front, after the maximum and at the end; it never wins
        x[at[0]] = 300.0
        x[[0, at[0] + 1, n - 1]] = np.nan
    else:
        x[list(at)] = 300.0
    return x


# ---- the table ------------------------------------------------------------------------------------------------------------------
def _factor(n: int, k: int):
    """n as a product of k factors >= 2, the first ones as small as they come, or None."""
    if k == 1:
        return (n,) if n >= 2 else None
    for f in range(2, int(n ** 0.5) + 1):
        if n % f == 0:
            rest = _factor(n // f, k - 1)
            if rest:
                return (f,) + rest
    return None


def wrap_rows(row_vecs: int) -> int:
    """The smallest number of rows of `row_vecs` vectors that leaves a whole vector for the second trip of a capped grid."""
    return CAP * BLOCK // row_vecs + 1


WIDTH_ROWS = (("bf16", 48, "vec16"), ("bf16", 44, "vec8"), ("bf16", 46, "vec4"), ("bf16", 45, "vec2"), ("u8", 45, "vec1"))
VIEW_OFFS = ((1, "vec2"), (2, "vec4"), (4, "vec8"))          # a bf16 view of 48-element rows, 1 / 2 / 4 elements into an allocation
TRANSPOSE_SHAPES = ((1, 1), (63, 65), (64, 64), (65, 63), (1, 130), (130, 1), (129, 200))


def _cases() -> list:
    out = []
    add = lambda *a, **k: out.append(Case(*a, **k))          # noqa: E731
    # -- 2-D and batched transposes
    for item in ("u8", "bf16", "f32", "i64"):
        for i, shp in enumerate(TRANSPOSE_SHAPES):
            add("transpose", "transpose" if i % 2 == 0 else "T", item, shp, leaf="tile64")
        add("transpose", "transpose", item, (65, 63), mis=(("in", 1),), leaf="tile64")
        add("transpose", "T", item, (63, 65), mis=(("in", 1),), leaf="tile64")
        for b in (1, 3):
            add("transpose", "transpose_3d_012", item, (b, 63, 65), leaf="tile64")
            add("transpose", "transpose_4d_0132", item, (b, 2, 65, 63), leaf="tile64")
        add("transpose", "transpose_3d_012", item, (3, 129, 200), mis=(("in", 1), ("out", 1)), leaf="tile64")
        add("transpose", "transpose_4d_0132", item, (3, 2, 65, 63), mis=(("in", 1), ("out", 1)), leaf="tile64")
    # -- row maps: every width by row length, then by view offset, per entry point
    for item, L, leaf in WIDTH_ROWS:
        add("row_map", "transpose_3d_021", item, (3, 5, L), leaf=leaf)
        add("row_map", "transpose_102", item, (5, 3, L), leaf=leaf)
        add("row_map", "transpose_4d_0213", item, (2, 3, 5, L), leaf=leaf)
        for rep in (1, 2, 5):
            add("row_map", "repeat_interleave_axis1", item, (2, 3, L), leaf=leaf, extra=(rep,))
    for off, leaf in VIEW_OFFS:
        add("row_map", "transpose_3d_021", "bf16", (3, 5, 48), mis=(("in", off),), leaf=leaf)
        add("row_map", "transpose_3d_021", "bf16", (3, 5, 48), mis=(("out", off),), leaf=leaf)
        add("row_map", "transpose_4d_0213", "bf16", (2, 3, 5, 48), mis=(("in", off), ("out", off)), leaf=leaf)
        add("row_map", "transpose_102", "bf16", (5, 3, 48), mis=(("in", off),), leaf=leaf)
        add("row_map", "repeat_interleave_axis1", "bf16", (2, 3, 48), mis=(("in", off),), leaf=leaf, extra=(2,))
    d0, d1 = _factor(wrap_rows(45), 2)
    add("row_map", "transpose_3d_021", "bf16", (d0, d1, 45), leaf="vec2", wrap=True)
    d0, d1, rep = _factor(wrap_rows(43), 3)
    add("row_map", "repeat_interleave_axis1", "bf16", (d0, d1, 43), leaf="vec2", wrap=True, extra=(rep,))
    d0, d1 = _factor(wrap_rows(1), 2)
    add("row_map", "transpose_3d_021", "bf16", (d0, d1, 8), leaf="vec16", wrap=True)
    # -- split_qkv: shape = (rows, q, k, v) elements
    for item, dims, leaf in (("bf16", (64, 64, 64), "vec16"), ("bf16", (64, 16, 16), "vec16"), ("bf16", (12, 4, 4), "vec8"), ("bf16", (6, 2, 2), "vec4"),
                             ("bf16", (5, 3, 3), "vec2"), ("f32", (3, 1, 1), "vec4"), ("f32", (6, 2, 4), "vec8"), ("u8", (5, 3, 3), "vec1"),
                             ("u8", (6, 2, 2), "vec2")):
        add("split_qkv", "split_qkv_batch", item, (7,) + dims, leaf=leaf)
    for name in ("qkv", "q", "k", "v"):
        add("split_qkv", "split_qkv_batch", "bf16", (7, 64, 64, 64), mis=((name, 1),), leaf="vec2")
    add("split_qkv", "split_qkv_batch", "bf16", (wrap_rows(11), 5, 3, 3), leaf="vec2", wrap=True)
    # -- gathers: shape = (table rows, hidden); extra = ids
    ids = (0, 6, 3, 3, 0)
    for item, L, leaf in WIDTH_ROWS + (("bf16", 64, "vec16"), ("bf16", 4096, "vec16")):
        add("gather", "embedding_lookup_batch", item, (7, L), leaf=leaf, extra=ids)
        add("gather", "gather_embeddings", item, (7, L), leaf=leaf, extra=ids)
        for tok in (0, 6):
            add("gather", "embedding_lookup", item, (7, L), leaf=leaf, extra=(tok,))
            add("gather", "embedding_lookup_ptr", item, (7, L), leaf=leaf, extra=(tok,))
        add("slice", "slice_rows_range_ptr", item, (7, L), leaf=leaf, extra=(2, 4))          # (start, count)
        add("slice", "slice_rows_range_ptr", item, (7, L), leaf=leaf, extra=(0, 7))
    for off, leaf in VIEW_OFFS:
        add("gather", "embedding_lookup_batch", "bf16", (7, 48), mis=(("table", off),), leaf=leaf, extra=ids)
        add("gather", "embedding_lookup_batch", "bf16", (7, 48), mis=(("out", off),), leaf=leaf, extra=ids)
        add("gather", "gather_embeddings", "bf16", (7, 48), mis=(("table", off),), leaf=leaf, extra=ids)
        add("gather", "embedding_lookup", "bf16", (7, 48), mis=(("table", off), ("out", off)), leaf=leaf, extra=(6,))
        add("gather", "embedding_lookup_ptr", "bf16", (7, 48), mis=(("table", off), ("out", off)), leaf=leaf, extra=(6,))
        add("slice", "slice_rows_range_ptr", "bf16", (7, 48), mis=(("table", off),), leaf=leaf, extra=(2, 4))
        add("slice", "slice_rows_range_ptr", "bf16", (7, 48), mis=(("out", off),), leaf=leaf, extra=(2, 4))
    add("slice", "slice_rows_range_ptr", "bf16", (wrap_rows(45) + 2, 45), leaf="vec2", wrap=True, extra=(2, wrap_rows(45)))
    # -- head-major KV write: shape = (seq, hkv, D); extra = (cache heads, num_heads, max_seq, position)
    for item, D, leaf in WIDTH_ROWS:
        for hkv, g, expanded in ((2, 2, True), (2, 4, True), (2, 5, True), (2, 4, False), (1, 1, True)):
            hc = hkv * g if expanded else hkv
            for pos in (0, 9):
                add("kv_write", "kv_cache_update_gqa", item, (1, hkv, D), leaf=leaf, extra=(hc, hkv * g, 10, pos))
            add("kv_write", "kv_cache_prefill_gqa", item, (4, hkv, D), leaf=leaf, extra=(hc, hkv * g, 10, 3))
        for pos in (9, 10, 12):              # _ptr: the last row; the kernel skips a row at or beyond max_seq
            add("kv_write", "kv_cache_update_gqa_ptr", item, (1, 2, D), leaf=leaf, extra=(4, 4, 10, pos))
        add("kv_write", "kv_cache_prefill_gqa", item, (10, 2, D), leaf=leaf, extra=(4, 4, 10, 0))
    for off, leaf in VIEW_OFFS:
        add("kv_write", "kv_cache_prefill_gqa", "bf16", (4, 2, 48), mis=(("new_kv", off),), leaf=leaf, extra=(4, 4, 10, 6))
        add("kv_write", "kv_cache_update_gqa", "bf16", (1, 2, 48), mis=(("cache", off),), leaf=leaf, extra=(4, 4, 10, 9))
        add("kv_write", "kv_cache_update_gqa_ptr", "bf16", (1, 2, 48), mis=(("new_kv", off), ("cache", off)), leaf=leaf, extra=(4, 4, 10, 0))
    hc, seq = _factor(wrap_rows(45), 2)
    add("kv_write", "kv_cache_prefill_gqa", "bf16", (seq, hc, 45), leaf="vec2", wrap=True, extra=(hc, hc, seq + 1, 1))
    # -- sequence-major writes and plain copies (device-to-device copies: no kernel of the family, no leaf)
    for mis in ((), (("new_kv", 1),), (("cache", 1),), (("new_kv", 1), ("cache", 3))):
        add("seq_copy", "kv_cache_update", "bf16", (1, 2, 45), mis=mis, extra=(10, 0))
        add("seq_copy", "kv_cache_update", "bf16", (1, 2, 45), mis=mis, extra=(10, 9))
        add("seq_copy", "kv_cache_prefill", "bf16", (4, 2, 45), mis=mis, extra=(10, 6))
    for mis in ((), (("a", 1),), (("b", 1),)):
        add("seq_copy", "concat_axis0", "bf16", (3, 5, 9), mis=mis, extra=(2,))              # b has 2 rows
    for mis in ((), (("in", 1),), (("out", 1),)):
        add("seq_copy", "reshape_copy", "f32", (6, 35), mis=mis, extra=(10, 21))
    for mis in ((), (("in", 1),)):
        add("seq_copy", "reshape", "u8", (6, 35), mis=mis, extra=(-1, 14))
    # -- argmax: shape = (rows, n); extra = the kind of each row
    for item in ("f32", "f16", "bf16"):
        for n in ARGMAX_N:
            kinds = [k for k in ARGMAX_KINDS if argmax_places(k, n) is not None]
            leaf = "block1024" if n >= 16384 else "block256"
            for j in range(0, len(kinds), 3):
                trio = tuple((kinds + kinds)[j:j + 3])
                add("argmax", "argmax_rows" if (j // 3) % 2 == 0 else "argmax_sample", item, (3, n), leaf=leaf, extra=trio)
            for j, entry in enumerate(("argmax", "argmax_int", "sample_greedy", "argmax_rows", "argmax_rows_out")):
                add("argmax", entry, item, (1, n), leaf=leaf, extra=(kinds[(j + ARGMAX_N.index(n)) % len(kinds)],))
        add("argmax", "argmax_rows_out", item, (3, 257), mis=(("x", 1), ("out", 1)), leaf="block256", extra=("tie_ends", "nan", "tie_waves"))
    # -- paged cache write: shape = (tokens, hkv, D); extra = (num_blocks, block_size)
    for item in ("bf16", "f16"):
        for D in (64, 128):
            for bs in (1, 4, 16):
                add("paged_write", "reshape_and_cache" if bs != 4 else "copy_to_paged_cache", item, (9, 2, D), leaf="vec16", extra=(5 if bs > 1 else 12, bs))
    add("paged_write", "copy_to_paged_cache", "bf16", (9, 2, 64), mis=(("k", 8), ("v", 8), ("k_cache", 8), ("v_cache", 8)), leaf="vec16", extra=(5, 4))
    add("paged_write", "reshape_and_cache", "bf16", (CAP * BLOCK // 16 + 1, 1, 128), leaf="vec16", wrap=True, extra=(CAP * BLOCK // 256 + 1, 16))
    # -- scatter_last_token_logits: shape = (batch, vocab); extra = sequence lengths
    lens = (1, 3, 2)
    for item, vocab, leaf in (("f16", 1000, "vec16"), ("f16", 50257, "vec2"), ("f32", 50257, "vec4"), ("bf16", 24, "vec16"), ("bf16", 4104, "vec16"),
                              ("bf16", 44, "vec8"), ("f32", 1030, "vec8"), ("bf16", 2049, "vec2"), ("u8", 45, "vec1"), ("f32", 7, "vec4")):
        add("scatter_last", "scatter_last_token_logits", item, (3, vocab), leaf=leaf, extra=lens)
    add("scatter_last", "scatter_last_token_logits", "f16", (1, 1000), leaf="vec16", extra=(1,))
    for off, leaf in VIEW_OFFS:
        add("scatter_last", "scatter_last_token_logits", "f16", (3, 1000), mis=(("out", off),), leaf=leaf, extra=lens)
        add("scatter_last", "scatter_last_token_logits", "f16", (3, 1000), mis=(("logits", off),), leaf=leaf, extra=lens)
    # -- batching helpers
    add("position_ids", "prepare_position_ids", "i32", (5,), extra=((0, 1, 256, 257, 1), (1, 0, 1, 1, 0)))      # (input lengths, is_prefill)
    add("position_ids", "prepare_position_ids", "i32", (2,), extra=((257, 1), (0, 1)))
    for n in (1, 256, 257):
        for how in ("none", "once", "all"):
            for eos in (0, 50256):
                add("check_eos", "check_eos", "i32", (n,), extra=(how, eos))
    for n in (1, 2, 1000):
        add("cumsum", "compute_cumsum", "i32", (n,))
    add("batch_inputs", "prepare_batch_inputs", "i32", (3,), extra=((5, 1, 9), (), (7,)))
    return out


CASES = _cases()


def groups() -> dict:
    g: dict = {}
    for c in CASES:
        g.setdefault(f"{c.fam}-{c.entry}-{c.item}" + ("-wrap" if c.wrap else ""), []).append(c)
    return g


def off(c: Case, name: str) -> int:
    return dict(c.mis).get(name, 0)


# ---- operands -------------------------------------------------------------------------------------------------------------------
def operands(c: Case) -> dict:
    """name -> Op, in the order the GPU test uploads them."""
    rng = np.random.default_rng(_seed(c))
    it, s, e = c.item, c.shape, c.extra
    W = lambda shape, item=it: words(rng, item, shape)          # noqa: E731
    if c.fam == "transpose":
        ret = c.entry in ("transpose", "T")
        return {"in": Op(it, W(s), "in"), "out": Op(it, canary(it, s[:-2] + (s[-1], s[-2])), "ret" if ret else "out")}
    if c.fam == "row_map":
        if c.entry == "repeat_interleave_axis1":
            return {"in": Op(it, W(s), "in"), "out": Op(it, canary(it, (s[0], s[1] * e[0], s[2])), "ret")}
        oshape = (s[1], s[0], s[2]) if len(s) == 3 else (s[0], s[2], s[1], s[3])
        return {"in": Op(it, W(s), "in"), "out": Op(it, canary(it, oshape), "ret" if c.entry == "transpose_102" else "out")}
    if c.fam == "split_qkv":
        rows, q, k, v = s
        return {"qkv": Op(it, W((rows, q + k + v)), "in"), "q": Op(it, canary(it, (rows, q)), "out"), "k": Op(it, canary(it, (rows, k)), "out"),
                "v": Op(it, canary(it, (rows, v)), "out")}
    if c.fam == "gather":
        n = len(e)
        ops = {"table": Op(it, W(s), "in"), "out": Op(it, canary(it, (n, s[1])), "ret" if c.entry == "gather_embeddings" else "out")}
        if c.entry != "embedding_lookup":
            ops["ids"] = Op("i32", i32(e), "in")
        return ops
    if c.fam == "slice":
        return {"table": Op(it, W(s), "in"), "out": Op(it, canary(it, (e[1], s[1])), "out"), "start": Op("i32", i32(e[0]), "in")}
    if c.fam == "kv_write":
        hc, _, max_seq, pos = e
        ops = {"new_kv": Op(it, W(s), "in"), "cache": Op(it, W((hc, max_seq, s[2])), "inout", guard=4 * s[2])}       # room for a row 3 beyond the cache
        if c.entry.endswith("_ptr"):
            ops["pos"] = Op("i32", i32(pos), "in")
        return ops
    if c.fam == "seq_copy":
        if c.entry in ("kv_cache_update", "kv_cache_prefill"):
            return {"new_kv": Op(it, W(s), "in"), "cache": Op(it, W((e[0],) + s[1:]), "inout")}
        if c.entry == "concat_axis0":
            return {"a": Op(it, W(s), "in"), "b": Op(it, W((e[0],) + s[1:]), "in"), "out": Op(it, canary(it, (s[0] + e[0],) + s[1:]), "ret")}
        oshape = tuple(d if d != -1 else int(np.prod(s)) // -int(np.prod(e)) for d in e)
        return {"in": Op(it, W(s), "in"), "out": Op(it, canary(it, oshape), "out" if c.entry == "reshape_copy" else "ret")}
    if c.fam == "argmax":
        x = np.stack([float_words(argmax_row(rng, kind, s[1]), it) for kind in e])
        given = c.entry == "argmax_rows_out"
        return {"x": Op(it, x, "in"), "out": Op("i64" if c.entry == "argmax" else "i32", canary("i64" if c.entry == "argmax" else "i32", (s[0],)),
                                                 "out" if given else "ret")}
    if c.fam == "paged_write":
        nb, bs = e
        tokens, hkv, D = s
        inner = 1 + rng.permutation(nb * bs - 2)                            # scattered order, no slot twice
        slots = inner[:tokens].astype(np.int32)
        slots[0], slots[tokens // 2] = 0, nb * bs - 1                       # the first slot of block 0, the last slot of the last block
        slots[[2, tokens - 2]] = -1                                         # padding tokens: skipped (the last token is a live one)
        block = hkv * bs * D                                                # an unguarded negative slot lands at most one block before the cache
        return {"k": Op(it, W(s), "in"), "v": Op(it, W(s), "in"), "k_cache": Op(it, W((nb, hkv, bs, D)), "inout", guard=block),
                "v_cache": Op(it, W((nb, hkv, bs, D)), "inout", guard=block), "slots": Op("i32", slots, "in")}
    if c.fam == "scatter_last":
        lens = np.asarray(e, np.int32)
        return {"logits": Op(it, W((int(lens.sum()), s[1])), "in"), "out": Op(it, canary(it, s), "out"),
                "start": Op("i32", i32(np.cumsum(lens) - lens), "in"), "lens": Op("i32", lens, "in")}
    if c.fam == "position_ids":
        lens, pf = np.asarray(e[0], np.int32), np.asarray(e[1], np.int32)
        start = (np.cumsum(lens + 2) - lens - 1).astype(np.int32)           # a gap before every sequence: positions of no sequence
        ctx = rng.integers(1000, 5000, size=lens.size).astype(np.int32)
        total = int(start[-1] + lens[-1] + 1)
        return {"start": Op("i32", start, "in"), "ctx": Op("i32", ctx, "in"), "pf": Op("i32", pf, "in"), "lens": Op("i32", lens, "in"),
                "out": Op("i32", np.zeros(total, np.int32), "ret")}            # the wrapper hands out zeros: the canary of this op
    if c.fam == "check_eos":
        how, eos = e
        t = rng.integers(1, 50000, size=s).astype(np.int32)
        if how == "once":
            t[s[0] - 1] = eos
        elif how == "all":
            t[:] = eos
        return {"tokens": Op("i32", t, "in"), "out": Op("i32", canary("i32", s), "ret")}
    if c.fam == "cumsum":
        x = rng.integers(0, 4, size=s).astype(np.int32)                     # zeros among the lengths
        x[0] = 3
        if s[0] > 2:
            x[[1, s[0] // 2]] = 0
        return {"in": Op("i32", x, "in"), "out": Op("i32", canary("i32", s), "ret")}
    assert c.fam == "batch_inputs", c.fam
    return {"out": Op("i32", canary("i32", (sum(len(t) for t in e),)), "ret")}


def outputs(c: Case, ops: dict) -> list:
    return [n for n, o in ops.items() if o.role != "in"]


# ---- the oracle -----------------------------------------------------------------------------------------------------------------
def expected(c: Case, ops: dict) -> dict:
    """Every word of every output, by NumPy indexing on the input words."""
    w = {n: o.words for n, o in ops.items()}
    s, e = c.shape, c.extra
    if c.fam == "transpose":
        return {"out": np.ascontiguousarray(np.swapaxes(w["in"], -1, -2))}
    if c.fam == "row_map":
        if c.entry == "repeat_interleave_axis1":
            return {"out": np.repeat(w["in"], e[0], axis=1)}
        return {"out": np.ascontiguousarray(np.swapaxes(w["in"], -3, -2))}
    if c.fam == "split_qkv":
        q, k, v = np.split(w["qkv"], [s[1], s[1] + s[2]], axis=1)
        return {"q": np.ascontiguousarray(q), "k": np.ascontiguousarray(k), "v": np.ascontiguousarray(v)}
    if c.fam == "gather":
        return {"out": np.take(w["table"], np.asarray(e), axis=0)}
    if c.fam == "slice":
        return {"out": w["table"][e[0]:e[0] + e[1]].copy()}
    if c.fam == "kv_write":
        hc, _, max_seq, pos = e
        cache = w["cache"].copy()
        per_head = np.repeat(w["new_kv"], hc // s[1], axis=1)               # [seq, hc, D]: each KV head serves hc / hkv cache heads in a row
        rows = np.arange(pos, pos + w["new_kv"].shape[0])
        ok = rows < max_seq                                                  # rows beyond the cache are skipped
        cache[:, rows[ok]] = np.swapaxes(per_head[ok], 0, 1)
        return {"cache": cache}
    if c.fam == "seq_copy":
        if c.entry in ("kv_cache_update", "kv_cache_prefill"):
            cache = w["cache"].copy()
            cache[e[1]:e[1] + s[0]] = w["new_kv"]
            return {"cache": cache}
        if c.entry == "concat_axis0":
            return {"out": np.concatenate([w["a"], w["b"]], axis=0)}
        return {"out": w["in"].reshape(ops["out"].words.shape).copy()}
    if c.fam == "argmax":
        x = words_float(w["x"], c.item)
        return {"out": np.asarray([argmax_rule(r) for r in x]).astype(WORD[ops["out"].item])}
    if c.fam == "paged_write":
        bs = e[1]
        res = {}
        live = np.flatnonzero(w["slots"] >= 0)
        sl = w["slots"][live]
        for src, name in (("k", "k_cache"), ("v", "v_cache")):
            cache = w[name].copy()                                           # [nb, hkv, bs, D]
            by_slot = np.swapaxes(cache, 1, 2).reshape(-1, s[1], s[2]).copy()  # [nb * bs, hkv, D]: NumPy's own view of "slot"
            by_slot[sl] = w[src][live]
            res[name] = np.ascontiguousarray(np.swapaxes(by_slot.reshape(e[0], bs, s[1], s[2]), 1, 2))
        return res
    if c.fam == "scatter_last":
        last = np.cumsum(w["lens"]) - 1
        return {"out": np.take(w["logits"], last, axis=0)}
    if c.fam == "position_ids":
        out = ops["out"].words.copy()
        for st, cx, pf, n in zip(w["start"], w["ctx"], w["pf"], w["lens"]):
            out[st:st + n] = np.arange(n) if pf else cx
        return {"out": out}
    if c.fam == "check_eos":
        return {"out": (w["tokens"] == e[1]).astype(np.int32)}
    if c.fam == "cumsum":
        return {"out": np.concatenate([[0], np.cumsum(w["in"])[:-1]]).astype(np.int32)}
    assert c.fam == "batch_inputs"
    return {"out": np.asarray([t for seq in e for t in seq], np.int32)}


# ---- the plan -------------------------------------------------------------------------------------------------------------------
PLAN_OP = {"transpose": None, "row_map": None, "split_qkv": "split_qkv", "gather": "embedding_lookup", "slice": "slice_rows", "kv_write": "kv_cache_write",
           "argmax": "argmax", "paged_write": "paged_cache_write", "scatter_last": "scatter_last_logits"}


def plan_args(c: Case):
    """(op, rows, row_bytes, itemsize, names of the operands whose addresses the launcher tests, keywords) for
    ops.tensor_op_plan / tensor_op_grid, or None where the path has no leaf."""
    s, e, isz = c.shape, c.extra, ITEM[c.item]
    if c.fam == "transpose":
        if len(s) == 2:
            return "transpose_2d", s[0], s[1] * isz, isz, (), {}
        return "transpose_batched", s[-2], s[-1] * isz, isz, (), {"batch": int(np.prod(s[:-2]))}
    if c.fam == "row_map":
        if c.entry == "repeat_interleave_axis1":
            return "repeat_interleave", s[0] * s[1] * e[0], s[2] * isz, isz, ("in", "out"), {}
        return "transpose_3d_021", s[-3] * s[-2], s[-1] * isz, isz, ("in", "out"), {}         # 4d_0213: one such launch per slab
    if c.fam == "split_qkv":
        return "split_qkv", s[0], sum(s[1:]) * isz, isz, ("qkv", "q", "k", "v"), {"widths": tuple(d * isz for d in s[1:])}
    if c.fam == "gather":
        return "embedding_lookup", len(e), s[1] * isz, isz, ("table", "out"), {}
    if c.fam == "slice":
        return "slice_rows", e[1], s[1] * isz, isz, ("table", "out"), {}
    if c.fam == "kv_write":
        return "kv_cache_write", s[0] * e[0], s[2] * isz, isz, ("new_kv", "cache"), {}
    if c.fam == "argmax":
        return "argmax", s[0], s[1] * isz, isz, (), {}
    if c.fam == "paged_write":
        return "paged_cache_write", s[0] * s[1], s[2] * isz, isz, (), {}
    if c.fam == "scatter_last":
        return "scatter_last_logits", s[0], s[1] * isz, isz, ("logits", "out"), {}
    return None


def vec_bytes(c: Case) -> int:
    return int(c.leaf[3:]) if c.leaf and c.leaf.startswith("vec") else ITEM[c.item]


def launches(c: Case) -> int:
    """Launches the entry point makes: transpose_4d_0213 starts one row map per slab."""
    return c.shape[0] if c.entry == "transpose_4d_0213" else 1


# ---- planted errors --------------------------------------------------------------------------------------------------------------
def _main(c: Case) -> str:
    return {"split_qkv": "k", "kv_write": "cache", "paged_write": "k_cache"}.get(c.fam, "cache" if c.entry.startswith("kv_cache") else "out")


def _rows(a: np.ndarray) -> np.ndarray:
    return a.reshape(-1, a.shape[-1] if a.ndim > 1 else 1)


def applicable(c: Case, ops: dict) -> list:
    """The planted errors that can show on this case, decided from the case alone."""
    s, e = c.shape, c.extra
    got = []
    rows = _rows(ops[_main(c)].words)
    row_family = c.fam in ("row_map", "split_qkv", "gather", "slice", "kv_write", "paged_write", "scatter_last", "seq_copy")
    if c.fam == "transpose":
        th, tw = s[-2] % 64, s[-1] % 64
        if (th >= 2 and s[-1] >= 2) or (tw >= 2 and s[-2] >= 2):
            got.append("swap_in_ragged_tile")
    if c.fam not in ("argmax", "batch_inputs") and rows.shape[0] >= 2 and (c.fam != "check_eos" or e[0] == "once"):
        got.append("row_off_by_one")
    if row_family and rows.shape[0] >= 2 and rows.shape[1] >= 2:
        got.append("wrong_width_stride")
    written = c.fam != "kv_write" or e[3] < e[2]          # a _ptr position beyond the cache writes nothing
    if (row_family or c.fam == "check_eos") and written:
        got.append("drop_last_vector")
    if c.wrap:
        got.append("drop_second_trip")
    if c.fam == "kv_write":
        if e[0] // s[1] >= 2 and s[1] >= 2 and written:
            got.append("head_mod_for_div")
        if e[3] < e[2]:
            got.append("position_plus_one")
    if c.fam == "seq_copy" and c.entry.startswith("kv_cache"):
        got.append("position_plus_one")
    if c.entry == "repeat_interleave_axis1" and e[0] >= 2 and s[1] >= 2:
        got.append("tile_for_repeat")
    if c.fam == "paged_write":
        got.append("k_v_exchanged")
        if e[1] >= 2:
            got.append("slot_div_mod_exchanged")
    if c.fam == "scatter_last" and s[0] >= 2:
        got.append("start_plus_len")
    if c.fam == "cumsum":
        got.append("inclusive_sum")
    if c.fam == "argmax":
        if any(k.startswith("tie") or k in ("pos_inf_tie", "zeros") for k in e):
            got.append("highest_index_on_ties")
        if "wave1" in e:
            got.append("first_wave_only")
        if "nan" in e:
            got.append("nan_wins")
    return got


def mutate(c: Case, name: str, ops: dict, exp: dict) -> dict:
    """The oracle's output with one planted error."""
    s, e = c.shape, c.extra
    out = {k: v.copy() for k, v in exp.items()}
    m = _main(c)
    before = ops[m].words
    if name == "swap_in_ragged_tile":              # a ragged tile's square corner is left untransposed
        src, dst = ops["in"].words.reshape((-1,) + s[-2:]), out["out"].reshape((-1, s[-1], s[-2]))
        for by in range(0, s[-2], 64):
            for bx in range(0, s[-1], 64):
                h, w_ = min(64, s[-2] - by), min(64, s[-1] - bx)
                if h < 64 or w_ < 64:
                    k = min(h, w_)
                    dst[:, bx:bx + k, by:by + k] = src[:, by:by + k, bx:bx + k]
    elif name == "row_off_by_one":
        out[m] = np.roll(_rows(exp[m]), 1, axis=0).reshape(exp[m].shape)
    elif name == "wrong_width_stride":             # rows found with half the row stride
        flat, L = exp[m].reshape(-1), _rows(exp[m]).shape[1]
        out[m] = flat[np.arange(flat.size // L)[:, None] * (L // 2) + np.arange(L)].reshape(exp[m].shape)
    elif name == "drop_last_vector":               # the last vector of every row keeps what the buffer held
        v = max(1, vec_bytes(c) // ITEM[ops[m].item])
        if out[m].ndim == 1:
            out[m][-v:] = before[-v:]
        else:
            _rows(out[m])[:, -v:] = _rows(before)[:, -v:]
    elif name == "drop_second_trip":               # work items beyond grid * 256 are never visited
        v = max(1, vec_bytes(c) // ITEM[ops[m].item])
        if c.fam in ("kv_write", "paged_write"):   # items index the source: token-major; undo the last rows' writes
            again = expected(c, _truncated(c, ops, CAP * BLOCK * v))
            out = {k: again[k] for k in out}
        elif c.fam == "split_qkv":
            rows_done = CAP * BLOCK * v // sum(s[1:])
            for k in out:
                out[k][rows_done + 1:] = ops[k].words[rows_done + 1:]
            out["v"][rows_done, -1:] = ops["v"].words[rows_done, -1:]
        else:
            out[m].reshape(-1)[CAP * BLOCK * v:] = before.reshape(-1)[CAP * BLOCK * v:]
    elif name == "head_mod_for_div":
        hc, _, max_seq, pos = e
        heads = np.arange(hc) % s[1]
        out[m][:, pos:pos + s[0]] = np.swapaxes(ops["new_kv"].words[:, heads], 0, 1)[:, :max_seq - pos]
    elif name == "tile_for_repeat":
        out[m] = np.tile(ops["in"].words, (1, e[0], 1))
    elif name == "position_plus_one":
        pos = e[3] if c.fam == "kv_write" else e[1]
        axis = 1 if c.fam == "kv_write" else 0
        moved = before.copy()
        new = np.take(exp[m], np.arange(pos, pos + s[0]), axis=axis)
        keep = moved.shape[axis] - (pos + 1)
        idx = [slice(None)] * moved.ndim
        idx[axis] = slice(pos + 1, pos + 1 + s[0])
        moved[tuple(idx)] = np.take(new, np.arange(min(s[0], keep)), axis=axis)
        out[m] = moved
    elif name == "k_v_exchanged":
        out["k_cache"], out["v_cache"] = _paged(c, ops, "v", "k_cache"), _paged(c, ops, "k", "v_cache")
    elif name == "slot_div_mod_exchanged":
        out["k_cache"], out["v_cache"] = _paged(c, ops, "k", "k_cache", swap=True), _paged(c, ops, "v", "v_cache", swap=True)
    elif name == "start_plus_len":
        lens = ops["lens"].words
        out[m] = np.take(ops["logits"].words, np.cumsum(lens) % int(lens.sum()), axis=0)
    elif name == "inclusive_sum":
        out[m] = np.cumsum(ops["in"].words).astype(np.int32)
    else:
        x = words_float(ops["x"].words, c.item)
        B = argmax_block(s[1])
        kw = {"highest_index_on_ties": {"ties": "highest"}, "first_wave_only": {"keep": (np.arange(s[1]) % B) // 64 == 0}, "nan_wins": {"nan_wins": True}}[name]
        out[m] = np.asarray([argmax_rule(r, **kw) for r in x]).astype(exp[m].dtype)
    return out


def _truncated(c: Case, ops: dict, items: int) -> dict:
    """The operands of a token-major writer with the tokens of the second trip taken away (their slots / rows never written)."""
    s = c.shape
    per_token = int(np.prod(s[1:])) if c.fam == "paged_write" else c.extra[0] * s[2]
    done = items // per_token                      # whole tokens of the first trip; the partial one counts as not written
    cut = dict(ops)
    if c.fam == "paged_write":
        slots = ops["slots"].words.copy()
        slots[done:] = -1
        cut["slots"] = Op("i32", slots, "in")
        return cut
    cut["new_kv"] = Op(c.item, ops["new_kv"].words[:done], "in")
    return cut


def _paged(c: Case, ops: dict, src: str, dst: str, swap: bool = False) -> np.ndarray:
    cache = ops[dst].words.copy()
    nb, bs = c.extra
    for t, slot in enumerate(ops["slots"].words):
        if slot < 0:
            continue
        b, o = divmod(int(slot), bs)
        if swap:
            b, o = o, b
        if b < nb and o < bs:
            cache[b, :, o] = ops[src].words[t]
    return cache


def wrap_items(c: Case) -> int:
    """Work items (vectors) of a grid-stride case, from the shapes of its operands."""
    ops_shape = {"row_map": lambda: int(np.prod(c.shape)) * (c.extra[0] if c.extra else 1), "split_qkv": lambda: c.shape[0] * sum(c.shape[1:]),
                 "slice": lambda: c.extra[1] * c.shape[1], "kv_write": lambda: c.shape[0] * c.extra[0] * c.shape[2],
                 "paged_write": lambda: int(np.prod(c.shape))}[c.fam]()
    return ops_shape * ITEM[c.item] // vec_bytes(c)
