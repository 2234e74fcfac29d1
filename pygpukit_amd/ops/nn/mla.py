"""[build-defined] Multi-head latent attention (DeepSeek-V2 / V3 / R1, Kimi-K2) in its absorbed decode form.

Latent cache [max_seq, 576], one row for ALL heads: row r = [c_r (512): the RMS-normed compressed latent | kpe_r (64): the roped
shared key].  The same 512 latent columns are the keys and the values.

  mla_cache_write / _ptr        kv_a [S, 576] (kv_a_proj_with_mqa's output) -> rows position ..: rmsnorm of the first 512 columns,
                                rotate-half RoPE of the last 64 at rows position + s of cos / sin [max_pos, 64]; one launch, the bits
                                of rmsnorm + rope_inplace (rope_inplace_f32table for float32 tables) + a copy
  sdpa_mla_fixed_cache / _ptr   q [q_len, H, 576] = [q_abs | q_pe] with W_UK absorbed -> out [q_len, H, 512]:
                                out[i, h] = sum_r softmax_r(scale <q[i, h], cache[r]>) cache[r, :512], r <= context_len - q_len + i
  sdpa_mla_plan                 ("mla_latent_mfma", query-tile columns, cache chunks); needs no GPU work
and a prompt chunk in the decompressed (textbook) form at qk_nope 128 / qk_rope 64 / v 128, 3.4 times less arithmetic than the above:
  sdpa_mla_prefill              q_nope [S, H, 128], q_pe [S, H, 64], kv [T, H, 256] = kv_b_proj of the latent rows -> out [S, H, 128]
  sdpa_mla_prefill_plan         ("mla_prefill_mfma", (query tiles, heads)); needs no GPU work

bfloat16 / float16, 1 <= H <= 128.  `scale` is required and positive: the model's is mscale^2 / sqrt(192), not 1 / sqrt(576)."""

from __future__ import annotations

import ctypes as C

from pygpukit_amd import _hip
from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import as_dtype, bfloat16, float16, float32, int32
from pygpukit_amd.core.factory import zeros
from pygpukit_amd.ops._common import call

LATENT, ROPE, WIDTH, MAX_HEADS = 512, 64, 576, 128
PREFILL_NOPE, PREFILL_V = 128, 128          # the head dims sdpa_mla_prefill is built for
_ws_cache: dict[tuple[int, int, int], GPUArray] = {}


def _check_write(kv_a, gamma, cos, sin, cache, name: str) -> int:
    if kv_a.ndim != 2 or kv_a.shape[1] != WIDTH or kv_a.dtype not in (bfloat16, float16):
        raise ValueError(f"{name}: kv_a must be bfloat16 / float16 [S, {WIDTH}], got {kv_a.shape}/{kv_a.dtype}")
    if cache.ndim != 2 or cache.shape[1] != WIDTH or cache.dtype != kv_a.dtype:
        raise ValueError(f"{name}: cache must be {kv_a.dtype} [max_seq, {WIDTH}], got {cache.shape}/{cache.dtype}")
    if gamma.shape != (LATENT,) or gamma.dtype != kv_a.dtype:
        raise ValueError(f"{name}: gamma must be {kv_a.dtype} [{LATENT}], got {gamma.shape}/{gamma.dtype}")
    if cos.ndim != 2 or cos.shape[1] != ROPE or sin.shape != cos.shape or cos.dtype != sin.dtype or cos.dtype not in (float32, kv_a.dtype):
        raise ValueError(f"{name}: cos / sin must be float32 or {kv_a.dtype} [max_pos, {ROPE}], got {cos.shape}/{cos.dtype} and "
                         f"{sin.shape}/{sin.dtype}")
    return int(cos.dtype == float32)


def mla_cache_write(kv_a: GPUArray, gamma: GPUArray, cos: GPUArray, sin: GPUArray, cache: GPUArray, position: int, eps: float = 1e-6) -> None:
    """kv_a [S, 576] -> rows position .. position + S - 1 of the latent cache [max_seq, 576]."""
    f32_table = _check_write(kv_a, gamma, cos, sin, cache, "mla_cache_write")
    s = kv_a.shape[0]
    if position < 0 or position + s > cache.shape[0] or position + s > cos.shape[0]:
        raise ValueError(f"mla_cache_write: rows {position}..{position + s - 1} outside the cache of {cache.shape[0]} rows or the table of "
                         f"{cos.shape[0]}")
    call("pgk_mla_cache_write", kv_a._p, gamma._p, cos._p, sin._p, cache._p, s, cache.shape[0], cos.shape[0], float(eps), int(position), None,
         f32_table, kv_a.dtype.code, None)


def mla_cache_write_ptr(kv_a: GPUArray, gamma: GPUArray, cos: GPUArray, sin: GPUArray, cache: GPUArray, position_buf: GPUArray,
                        eps: float = 1e-6) -> None:
    """mla_cache_write (a decode step's single row, or any S) with the position read from a device int32 (graph replay); a row
    outside the cache or the table is not written."""
    f32_table = _check_write(kv_a, gamma, cos, sin, cache, "mla_cache_write_ptr")
    if position_buf.dtype != int32:
        raise ValueError("mla_cache_write_ptr: position_buf must be int32")
    call("pgk_mla_cache_write", kv_a._p, gamma._p, cos._p, sin._p, cache._p, kv_a.shape[0], cache.shape[0], cos.shape[0], float(eps), 0,
         position_buf._p, f32_table, kv_a.dtype.code, None)


def _check_sdpa(q, cache, out, scale, name: str) -> tuple[int, int, int]:
    if q.ndim != 3 or q.shape[2] != WIDTH or q.dtype not in (bfloat16, float16):
        raise ValueError(f"{name}: q must be bfloat16 / float16 [q_len, H, {WIDTH}], got {q.shape}/{q.dtype}")
    q_len, heads, _ = q.shape
    if cache.ndim != 2 or cache.shape[1] != WIDTH or cache.dtype != q.dtype:
        raise ValueError(f"{name}: cache must be {q.dtype} [max_seq, {WIDTH}], got {cache.shape}/{cache.dtype}")
    if out.shape != (q_len, heads, LATENT) or out.dtype != q.dtype:
        raise ValueError(f"{name}: out must be {q.dtype} [{q_len}, {heads}, {LATENT}], got {out.shape}/{out.dtype}")
    if not 1 <= heads <= MAX_HEADS or not 1 <= q_len <= cache.shape[0]:
        raise ValueError(f"{name}: needs 1 <= H <= {MAX_HEADS} and 1 <= q_len <= max_seq, got H {heads}, q_len {q_len}, max_seq {cache.shape[0]}")
    if not scale > 0:
        raise ValueError(f"{name}: scale must be positive (the model's mscale^2 / sqrt(192) has no default), got {scale}")
    return heads, q_len, cache.shape[0]


def _workspace(heads: int, q_len: int, max_seq: int):
    key = (heads, q_len, max_seq)
    if key not in _ws_cache:
        nbytes = _hip.load().pgk_sdpa_mla_workspace_bytes(heads, q_len, max_seq)
        _ws_cache[key] = GPUArray((nbytes // 4,), float32) if nbytes else None
    ws = _ws_cache[key]
    return ws._p if ws is not None else None


def sdpa_mla_fixed_cache(q: GPUArray, cache: GPUArray, out: GPUArray, context_len: int, scale: float) -> None:
    """Query row i of q [q_len, H, 576] sees cache rows 0 .. context_len - q_len + i; out [q_len, H, 512].  Rows at and beyond
    context_len are never read."""
    heads, q_len, max_seq = _check_sdpa(q, cache, out, scale, "sdpa_mla_fixed_cache")
    if context_len < q_len or context_len > max_seq:
        raise ValueError(f"sdpa_mla_fixed_cache: invalid context_len {context_len} (q_len {q_len}, cache rows {max_seq})")
    call("pgk_sdpa_mla_fixed_cache", q._p, cache._p, out._p, heads, q_len, max_seq, float(scale), int(context_len), None,
         _workspace(heads, q_len, max_seq), q.dtype.code, None)


def sdpa_mla_fixed_cache_ptr(q: GPUArray, cache: GPUArray, out: GPUArray, context_len_buf: GPUArray, scale: float) -> None:
    """As above with context_len read from a device int32 (graph replay) and clamped to the cache; the grid depends on max_seq only."""
    heads, q_len, max_seq = _check_sdpa(q, cache, out, scale, "sdpa_mla_fixed_cache_ptr")
    if context_len_buf.dtype != int32:
        raise ValueError("sdpa_mla_fixed_cache_ptr: context_len_buf must be int32")
    call("pgk_sdpa_mla_fixed_cache", q._p, cache._p, out._p, heads, q_len, max_seq, float(scale), 0, context_len_buf._p,
         _workspace(heads, q_len, max_seq), q.dtype.code, None)


def sdpa_mla_plan(num_heads: int, q_len: int, max_seq: int, dtype) -> tuple[str, int, int]:
    """("mla_latent_mfma", columns of a query tile, cache chunks) of sdpa_mla_fixed_cache for this shape; ValueError for what the op
    rejects.  One chunk: the kernel writes `out` itself; more: a merge launch follows."""
    lib = _hip.load()
    cols, chunks = C.c_int(0), C.c_int(0)
    plan = lib.pgk_sdpa_mla_plan(int(num_heads), int(q_len), int(max_seq), as_dtype(dtype).code, C.byref(cols), C.byref(chunks))
    if plan is None:
        msg = lib.pgk_last_error()
        raise ValueError(msg.decode(errors="replace") if msg else "sdpa_mla_plan: invalid call")
    return plan.decode(), cols.value, chunks.value


def sdpa_mla_prefill(q_nope: GPUArray, q_pe: GPUArray, kv: GPUArray, cache: GPUArray, out: GPUArray, kv_len: int, scale: float) -> None:
    """Causal attention of a prompt chunk in MLA's decompressed form (qk_nope 128, qk_rope 64, v 128), one launch:
    out[i, h] = sum_j softmax_j(scale (<q_nope[i, h], kv[j, h, :128]> + <q_pe[i, h], cache[j, 512:]>)) kv[j, h, 128:], j <= kv_len - S + i.
    q_nope [S, H, 128], q_pe [S, H, 64] (roped), kv [kv_len, H, 256] = kv_b_proj of latent rows 0 .. kv_len - 1, cache [max_seq, 576]
    (only the rope columns of rows below kv_len are read), out [S, H, 128].  kv_len > S: a cached prefix.  There is no KV split: a
    chunk of a few rows over a long prefix is one workgroup's walk per head - sdpa_mla_fixed_cache is the tool for small q_len."""
    name = "sdpa_mla_prefill"
    if q_nope.ndim != 3 or q_nope.shape[2] != PREFILL_NOPE or q_nope.dtype not in (bfloat16, float16):
        raise ValueError(f"{name}: q_nope must be bfloat16 / float16 [S, H, {PREFILL_NOPE}], got {q_nope.shape}/{q_nope.dtype}")
    q_len, heads, _ = q_nope.shape
    if q_pe.shape != (q_len, heads, ROPE) or q_pe.dtype != q_nope.dtype:
        raise ValueError(f"{name}: q_pe must be {q_nope.dtype} [{q_len}, {heads}, {ROPE}], got {q_pe.shape}/{q_pe.dtype}")
    if kv.shape != (kv_len, heads, PREFILL_NOPE + PREFILL_V) or kv.dtype != q_nope.dtype:
        raise ValueError(f"{name}: kv must be {q_nope.dtype} [{kv_len}, {heads}, {PREFILL_NOPE + PREFILL_V}], got {kv.shape}/{kv.dtype}")
    if cache.ndim != 2 or cache.shape[1] != WIDTH or cache.dtype != q_nope.dtype:
        raise ValueError(f"{name}: cache must be {q_nope.dtype} [max_seq, {WIDTH}], got {cache.shape}/{cache.dtype}")
    if out.shape != (q_len, heads, PREFILL_V) or out.dtype != q_nope.dtype:
        raise ValueError(f"{name}: out must be {q_nope.dtype} [{q_len}, {heads}, {PREFILL_V}], got {out.shape}/{out.dtype}")
    if not 1 <= heads <= MAX_HEADS or not 1 <= q_len <= kv_len <= cache.shape[0]:
        raise ValueError(f"{name}: needs 1 <= H <= {MAX_HEADS} and 1 <= S <= kv_len <= max_seq, got H {heads}, S {q_len}, kv_len {kv_len}, "
                         f"max_seq {cache.shape[0]}")
    if not scale > 0:
        raise ValueError(f"{name}: scale must be positive (the model's mscale^2 / sqrt(192) has no default), got {scale}")
    call("pgk_sdpa_mla_prefill", q_nope._p, q_pe._p, kv._p, cache._p, out._p, heads, q_len, int(kv_len), cache.shape[0], float(scale),
         q_nope.dtype.code, None)


def sdpa_mla_prefill_plan(num_heads: int, q_len: int, kv_len: int, dtype) -> tuple[str, tuple[int, int]]:
    """("mla_prefill_mfma", (query tiles of 128 rows, heads)) of sdpa_mla_prefill; ValueError for what the op rejects.  No GPU work."""
    lib = _hip.load()
    grid = (C.c_int * 2)()
    plan = lib.pgk_sdpa_mla_prefill_plan(int(num_heads), int(q_len), int(kv_len), as_dtype(dtype).code, grid)
    if plan is None:
        msg = lib.pgk_last_error()
        raise ValueError(msg.decode(errors="replace") if msg else "sdpa_mla_prefill_plan: invalid call")
    return plan.decode(), (grid[0], grid[1])


# ---- the paged latent cache: [num_blocks, block_size, 576], a page row being a row of the cache above (no head axis); block_tables
# [num_seqs, max_blocks_per_seq], context_lens [num_seqs] and slot_mapping [n_tokens] are ops.paged's int32 device arrays ----------
_paged_ws_cache: dict[tuple[int, int, int, int], GPUArray | None] = {}


def allocate_mla_cache(num_blocks: int, block_size: int, dtype=bfloat16) -> GPUArray:
    """[num_blocks, block_size, 576], zero-filled; any block_size >= 1."""
    dtype = as_dtype(dtype)
    if num_blocks < 1 or block_size < 1 or dtype not in (bfloat16, float16):
        raise ValueError(f"allocate_mla_cache: needs num_blocks >= 1, block_size >= 1 and bfloat16 / float16, got {num_blocks}, {block_size}, {dtype}")
    return zeros((num_blocks, block_size, WIDTH), dtype)


def _check_pages(cache, dtype, name: str) -> None:
    if cache.ndim != 3 or cache.shape[2] != WIDTH or cache.dtype != dtype:
        raise ValueError(f"{name}: cache must be {dtype} [num_blocks, block_size, {WIDTH}], got {cache.shape}/{cache.dtype}")


def mla_reshape_and_cache(kv_a: GPUArray, gamma: GPUArray, cos: GPUArray, sin: GPUArray, positions: GPUArray, cache: GPUArray,
                          slot_mapping: GPUArray, eps: float = 1e-6) -> None:
    """kv_a [n_tokens, 576] -> slot slot_mapping[t] of the pages: what mla_cache_write puts into row positions[t] of a contiguous cache,
    bit for bit (each token has its own position: a decode batch has one per sequence).  One launch; a negative slot writes nothing."""
    name = "mla_reshape_and_cache"
    if kv_a.ndim != 2 or kv_a.shape[1] != WIDTH or kv_a.dtype not in (bfloat16, float16):
        raise ValueError(f"{name}: kv_a must be bfloat16 / float16 [n_tokens, {WIDTH}], got {kv_a.shape}/{kv_a.dtype}")
    _check_pages(cache, kv_a.dtype, name)
    if gamma.shape != (LATENT,) or gamma.dtype != kv_a.dtype:
        raise ValueError(f"{name}: gamma must be {kv_a.dtype} [{LATENT}], got {gamma.shape}/{gamma.dtype}")
    if cos.ndim != 2 or cos.shape[1] != ROPE or sin.shape != cos.shape or cos.dtype != sin.dtype or cos.dtype not in (float32, kv_a.dtype):
        raise ValueError(f"{name}: cos / sin must be float32 or {kv_a.dtype} [max_pos, {ROPE}], got {cos.shape}/{cos.dtype} and "
                         f"{sin.shape}/{sin.dtype}")
    n = kv_a.shape[0]
    for label, a in (("positions", positions), ("slot_mapping", slot_mapping)):
        if a.dtype != int32 or a.ndim != 1 or a.shape[0] != n:
            raise ValueError(f"{name}: {label} must be int32 [{n}], got {a.shape}/{a.dtype}")
    call("pgk_mla_paged_cache_write", kv_a._p, gamma._p, cos._p, sin._p, positions._p, cache._p, slot_mapping._p, n, cache.shape[0],
         cache.shape[1], cos.shape[0], float(eps), int(cos.dtype == float32), kv_a.dtype.code, None)


def sdpa_mla_paged_plan(num_heads: int, q_len: int, num_seqs: int, max_context: int, dtype) -> tuple[str, tuple[int, int, int]]:
    """("mla_paged_mfma", (column tiles of 32 (query row, head) pairs, KV chunks, sequences)) of sdpa_mla_paged: a function of the
    shape and the bound alone, never of the lengths.  One chunk: the kernel writes `out` itself; more: a merge launch follows.
    ValueError for what the op rejects.  No GPU work."""
    lib = _hip.load()
    grid = (C.c_int * 3)()
    plan = lib.pgk_sdpa_mla_paged_plan(int(num_heads), int(q_len), int(num_seqs), int(max_context), as_dtype(dtype).code, grid)
    if plan is None:
        msg = lib.pgk_last_error()
        raise ValueError(msg.decode(errors="replace") if msg else "sdpa_mla_paged_plan: invalid call")
    return plan.decode(), (grid[0], grid[1], grid[2])


def sdpa_mla_paged(q: GPUArray, cache: GPUArray, block_tables: GPUArray, context_lens: GPUArray, out: GPUArray, max_context: int,
                   scale: float) -> None:
    """sdpa_mla_fixed_cache for a decode batch straight off the pages, one launch (plus the merge): q [num_seqs, q_len, H, 576],
    out [num_seqs, q_len, H, 512]; row i of sequence b sees rows 0 .. context_lens[b] - q_len + i of the pages block_tables[b] names.
    context_lens stays on the device (graph replay): max_context bounds it, sizes the KV split and clamps what the kernel reads.  A
    sequence with context_lens[b] == 0 is idle and its rows are zeros; so, on the device, is one with fewer rows than q_len, which the
    host refuses where it can see it (max_context < q_len).  Table entries beyond a sequence's last page are never read."""
    name = "sdpa_mla_paged"
    if q.ndim != 4 or q.shape[3] != WIDTH or q.dtype not in (bfloat16, float16):
        raise ValueError(f"{name}: q must be bfloat16 / float16 [num_seqs, q_len, H, {WIDTH}], got {q.shape}/{q.dtype}")
    num_seqs, q_len, heads, _ = q.shape
    _check_pages(cache, q.dtype, name)
    if out.shape != (num_seqs, q_len, heads, LATENT) or out.dtype != q.dtype:
        raise ValueError(f"{name}: out must be {q.dtype} [{num_seqs}, {q_len}, {heads}, {LATENT}], got {out.shape}/{out.dtype}")
    if block_tables.dtype != int32 or block_tables.ndim != 2 or block_tables.shape[0] != num_seqs:
        raise ValueError(f"{name}: block_tables must be int32 [{num_seqs}, max_blocks_per_seq], got {block_tables.shape}/{block_tables.dtype}")
    if context_lens.dtype != int32 or context_lens.ndim != 1 or context_lens.shape[0] != num_seqs:
        raise ValueError(f"{name}: context_lens must be int32 [{num_seqs}], got {context_lens.shape}/{context_lens.dtype}")
    if not 1 <= heads <= MAX_HEADS or num_seqs < 1 or not 1 <= q_len <= max_context:
        raise ValueError(f"{name}: needs 1 <= H <= {MAX_HEADS}, num_seqs >= 1 and 1 <= q_len <= max_context, got H {heads}, num_seqs {num_seqs}, "
                         f"q_len {q_len}, max_context {max_context}")
    if not scale > 0:
        raise ValueError(f"{name}: scale must be positive (the model's mscale^2 / sqrt(192) has no default), got {scale}")
    key = (heads, q_len, num_seqs, int(max_context))
    if key not in _paged_ws_cache:
        nbytes = _hip.load().pgk_sdpa_mla_paged_workspace_bytes(*key)
        _paged_ws_cache[key] = GPUArray((nbytes // 4,), float32) if nbytes else None
    ws = _paged_ws_cache[key]
    call("pgk_sdpa_mla_paged", q._p, cache._p, block_tables._p, context_lens._p, out._p, num_seqs, heads, q_len, cache.shape[0], cache.shape[1],
         block_tables.shape[1], int(max_context), float(scale), ws._p if ws is not None else None, q.dtype.code, None)


__all__ = ["mla_cache_write", "mla_cache_write_ptr", "sdpa_mla_fixed_cache", "sdpa_mla_fixed_cache_ptr", "sdpa_mla_plan",
           "sdpa_mla_prefill", "sdpa_mla_prefill_plan", "allocate_mla_cache", "mla_reshape_and_cache", "sdpa_mla_paged", "sdpa_mla_paged_plan"]
