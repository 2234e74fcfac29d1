"""[build-defined] Attention with T5's bucketed relative-position bias applied inside the attention kernels.

    out[h, i] = softmax_j(q[h, i] . k[h // rep, j] * scale + table[h, clamp(j - i, -R, R) + R], over ALL j) . v[h // rep]

The reference's T5Encoder materialises bias[1, H, S, S] = weight[bucket(j - i)] on the host and adds it to materialised
scores.  Attention here never holds the scores in memory, and the bidirectional bucket is constant for |j - i| >=
max_distance, so the whole bias of ANY sequence length is a table [H, 2R + 1] with R = max_distance (relpos_bias_table),
indexed by the clamped distance: delta is KEY position minus QUERY position.  bfloat16 / float16 at head_dim 64 / 128 run
the MFMA flash kernel (csrc/ops_flash.hip, FlashRelBias: the head's row staged in LDS, the score accumulators start from it);
float32, other head dims up to 256 and unaligned buffers one wave per row (csrc/ops_relbias.hip).  Contract: INTEGRATION.md."""

from __future__ import annotations

import numpy as np

from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import as_dtype, float32
from pygpukit_amd.core.factory import from_numpy
from pygpukit_amd.ops._common import call, check_out, validate_float


def relpos_bucket(relative_position, bidirectional: bool = True, num_buckets: int = 32, max_distance: int = 128) -> np.ndarray:
    """T5's bucket of relative_position = key position - query position (host arithmetic; the reference's
    T5Encoder._relative_position_bucket operation for operation, so the buckets are bit-identical; HF's
    T5Attention._relative_position_bucket gives the same buckets)."""
    relative_position = np.asarray(relative_position)
    ret = 0
    n = -relative_position
    if bidirectional:
        num_buckets //= 2
        ret += (n < 0).astype(np.int32) * num_buckets
        n = np.abs(n)
    else:
        n = np.maximum(n, 0)
    max_exact = num_buckets // 2
    is_small = n < max_exact
    with np.errstate(divide="ignore", invalid="ignore"):
        val_if_large = max_exact + (np.log(n.astype(np.float32) / max_exact + 1e-6) / np.log(max_distance / max_exact)
                                    * (num_buckets - max_exact)).astype(np.int32)
    val_if_large = np.minimum(val_if_large, num_buckets - 1)
    ret += np.where(is_small, n, val_if_large)
    return ret


def relpos_bias_table_host(weight, bidirectional: bool = True, max_distance: int = 128) -> np.ndarray:
    """weight [num_buckets, H] (relative_attention_bias.weight) -> float32 [H, 2R + 1], R = max_distance:
    table[h, delta + R] = weight[bucket(delta), h] for delta = key - query in [-R, R]."""
    w = np.asarray(weight, dtype=np.float32)
    if w.ndim != 2:
        raise ValueError(f"relpos_bias_table: weight must be [num_buckets, num_heads], got shape {w.shape}")
    radius = int(max_distance)
    if radius < 1:
        raise ValueError(f"relpos_bias_table: max_distance must be >= 1, got {max_distance}")
    buckets = relpos_bucket(np.arange(-radius, radius + 1), bidirectional, w.shape[0], radius)
    return np.ascontiguousarray(w[buckets].T)


def relpos_compute_bias_host(table, q_len: int, kv_len: int) -> np.ndarray:
    """table [H, 2R + 1] -> the dense bias [H, q_len, kv_len] it stands for: table[h, clamp(j - i, -R, R) + R]."""
    t = np.asarray(table)
    if t.ndim != 2 or t.shape[1] % 2 != 1:
        raise ValueError(f"relpos_compute_bias: table must be [H, 2R + 1], got shape {t.shape}")
    radius = t.shape[1] // 2
    delta = np.arange(int(kv_len))[None, :] - np.arange(int(q_len))[:, None]
    return t[:, np.clip(delta, -radius, radius) + radius]


def relpos_bias_table(weight, bidirectional: bool = True, max_distance: int = 128) -> GPUArray:
    """relpos_bias_table_host on the device: the `table` argument of sdpa_relbias.  weight: NumPy array or GPUArray."""
    if isinstance(weight, GPUArray):
        weight = weight.to_numpy()
    return from_numpy(relpos_bias_table_host(weight, bidirectional, max_distance))


def relpos_compute_bias(table: GPUArray, q_len: int, kv_len: int) -> GPUArray:
    """The dense float32 bias [H, q_len, kv_len] of a table, for tests and compositions that materialise the scores; expanded
    on the host."""
    return from_numpy(np.ascontiguousarray(relpos_compute_bias_host(table.to_numpy(), q_len, kv_len), dtype=np.float32))


def _check_relbias(q: GPUArray, k: GPUArray, v: GPUArray, out: GPUArray | None, table: GPUArray, hq: int, hkv: int, q_len: int, kv_len: int,
                   d: int, name: str) -> int:
    validate_float(q, name)
    if q.dtype != k.dtype or q.dtype != v.dtype:
        raise ValueError(f"{name}: Q/K/V must have same dtype")
    if out is not None and out.dtype != q.dtype:
        raise ValueError(f"{name}: out must have same dtype as Q")
    if hq <= 0 or hkv <= 0 or hq % hkv != 0:
        raise ValueError(f"{name}: n_heads mismatch (Hq={hq}, Hkv={hkv})")
    if min(q_len, kv_len, d) < 1:
        raise ValueError(f"{name}: needs q_len, kv_len, head_dim >= 1, got {q_len}, {kv_len}, {d}")
    if table.dtype != float32:
        raise ValueError(f"{name}: table must be float32, got {table.dtype}")
    if table.ndim != 2 or table.shape[0] != hq or table.shape[1] % 2 != 1:
        raise ValueError(f"{name}: table must be [{hq}, 2R + 1] (one row per query head), got shape {table.shape}")
    return table.shape[1] // 2


def sdpa_relbias(Q: GPUArray, K: GPUArray, V: GPUArray, table: GPUArray, scale: float = 0.0, *, out: GPUArray | None = None) -> GPUArray:
    """Q [Hq, q_len, D], K / V [Hkv, kv_len, D] (un-expanded GQA), table [Hq, 2R + 1] float32: attention over every key with
    table[h, clamp(j - i, -R, R) + R] added to the scaled scores; any q_len, kv_len >= 1.  scale <= 0 -> 1/sqrt(head_dim) (T5
    passes 1.0)."""
    if Q.ndim != 3 or K.ndim != 3 or V.ndim != 3:
        raise ValueError("sdpa_relbias expects 3D Q, K, V [heads, seq, head_dim]")
    hq, q_len, d = Q.shape
    hkv, kv_len = K.shape[0], K.shape[1]
    if K.shape != V.shape or K.shape[2] != d:
        raise ValueError(f"sdpa_relbias: K {K.shape} / V {V.shape} do not fit Q {Q.shape}")
    radius = _check_relbias(Q, K, V, out, table, hq, hkv, q_len, kv_len, d, "sdpa_relbias")
    o = check_out(out, (hq, q_len, d), Q.dtype, "sdpa_relbias")
    call("pgk_sdpa_relbias", Q._p, K._p, V._p, table._p, o._p, hq, hkv, q_len, kv_len, d, radius, float(scale), q_len * d, d, kv_len * d, d,
         q_len * d, d, Q.dtype.code, None)
    return o


def sdpa_relbias_strided(q: GPUArray, k: GPUArray, v: GPUArray, table: GPUArray, out: GPUArray, hq: int, hkv: int, q_len: int, kv_len: int,
                         d: int, q_strides, kv_strides, o_strides, scale: float = 0.0) -> None:
    """sdpa_relbias on [S,H,D]-layout (or any head/row-strided) buffers, written into `out`: strides are (head, row) in
    elements, so the [S, 3*H*D] output of a fused QKV projection is read in place."""
    radius = _check_relbias(q, k, v, out, table, hq, hkv, q_len, kv_len, d, "sdpa_relbias_strided")
    if any(int(x) < 0 for x in (*q_strides, *kv_strides, *o_strides)):
        raise ValueError("sdpa_relbias_strided: strides must be non-negative")
    call("pgk_sdpa_relbias", q._p, k._p, v._p, table._p, out._p, hq, hkv, q_len, kv_len, d, radius, float(scale), q_strides[0], q_strides[1],
         kv_strides[0], kv_strides[1], o_strides[0], o_strides[1], q.dtype.code, None)


def relbias_plan(head_dim: int, radius: int, dtype, aligned: bool = True) -> str:
    """"relbias_flash" (bfloat16 / float16, head_dim 64 / 128, radius <= 1024, aligned buffers) or "relbias_rows"; needs no device."""
    from pygpukit_amd import _hip

    lib = _hip.load()
    plan = lib.pgk_relbias_plan(int(head_dim), int(radius), as_dtype(dtype).code, int(bool(aligned)))
    if plan is None:
        msg = lib.pgk_last_error()
        raise ValueError(msg.decode(errors="replace") if msg else f"relbias_plan: invalid call head_dim={head_dim} radius={radius} dtype={dtype}")
    return plan.decode()


__all__ = ["relpos_bucket", "relpos_bias_table", "relpos_bias_table_host", "relpos_compute_bias", "relpos_compute_bias_host", "sdpa_relbias",
           "sdpa_relbias_strided", "relbias_plan"]
