"""Restated oracle of the Mixture-of-Experts path (reference: native/ops/moe/topk_kernels.cuh, permute_kernels.cuh,
moe_kernels.cuh, native/ops/matmul/gemm/w8a16_bf16/sm120/grouped_gemm.cu and src/pygpukit/llm/layers/moe.py).

  routing      top-k of each logits row, descending, the lowest expert index first among equal values (the strict '>'
               scan of topk_with_indices_kernel); NaN ranks as -inf; then softmax over the k selected values in fp32
               (max, exp(x - max) summed in order, times 1/sum) - Qwen3-MoE's softmax-then-renormalise
  permutation  a STABLE sort of the flat (token * k + slot) entries by expert: this project's documented order (the
               reference's order within an expert is whatever atomicAdd produced)
  scatter      out[t] = sum over slot, in slot order, of w[t, slot] * y[reverse_perm[t * k + slot]] in fp32
  grouped GEMM C[r] = A[r] . W[e_r]^T, fp8 weights dequantised as lut[code] * float(scale) in fp32 with no bf16
               rounding (grouped_gemm.cu:53-68), fp32 accumulation.  The GPU's MFMA kernels round the dequantised
               weight to bf16 first: at most 2^-9 relative per weight, inside the 1e-2 bar of the tests.

RefMoE plugs into oracle.cpu_ref.RefBlock / RefModel as the `mlp`."""

from __future__ import annotations

import numpy as np

from oracle import cpu_ref as O

TILE_ROWS = 128


def topk_indices(logits: np.ndarray, k: int) -> np.ndarray:
    """[T, E] -> int32 [T, k]: value descending, expert ascending among equal values; NaN ranks as -inf."""
    v = np.where(np.isnan(logits), -np.inf, np.asarray(logits, np.float32))
    E = v.shape[1]
    out = np.empty((v.shape[0], k), np.int32)
    for t in range(v.shape[0]):
        order = np.lexsort((np.arange(E), -v[t]))
        out[t] = order[:k]
    return out


def softmax_k(values: np.ndarray) -> np.ndarray:
    """softmax_topk over each row, fp32 operations in the kernel's order."""
    x = np.asarray(values, np.float32)
    out = np.empty_like(x)
    for t in range(x.shape[0]):
        mx = np.float32(x[t].max())
        with np.errstate(invalid="ignore"):        # a row of -inf gives NaN weights, as the kernel's does
            e = np.exp((x[t] - mx).astype(np.float32)).astype(np.float32)
        s = np.float32(0.0)
        for v in e:
            s = np.float32(s + v)
        out[t] = e * np.float32(np.float32(1.0) / s)
    return out


def topk_softmax(logits: np.ndarray, k: int, bf16: bool) -> tuple[np.ndarray, np.ndarray]:
    """(weights [T, k] fp32 (bf16-rounded when the logits are bf16), indices [T, k])."""
    idx = topk_indices(logits, k)
    vals = np.take_along_axis(np.asarray(logits, np.float32), idx, axis=1)
    w = softmax_k(vals)
    return (O.bf16_round(w) if bf16 else w), idx


def topk_margin(logits: np.ndarray, k: int) -> float:
    """Smallest gap between the k-th and (k+1)-th largest logit of any row (inf when k == E)."""
    s = -np.sort(-np.asarray(logits, np.float64), axis=1)
    return float(np.min(s[:, k - 1] - s[:, k])) if s.shape[1] > k else float("inf")


def permutation(indices: np.ndarray, E: int):
    """Stable counting sort: (counts [E], offsets [E+1], permute [T*k], reverse [T*k]).  Ids outside [0, E) are not
    placed: their reverse entry is -1 and permute is -1 past offsets[E]."""
    flat = np.asarray(indices, np.int64).ravel()
    valid = (flat >= 0) & (flat < E)
    counts = np.bincount(flat[valid], minlength=E).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    key = np.where(valid, flat, E)
    order = np.argsort(key, kind="stable")
    n_valid = int(valid.sum())
    perm = np.full(flat.size, -1, np.int32)
    perm[:n_valid] = order[:n_valid]
    rev = np.full(flat.size, -1, np.int32)
    rev[order[:n_valid]] = np.arange(n_valid, dtype=np.int32)
    return counts, offsets, perm, rev


def permutation_loop(indices, E: int):
    """The same, as the plainest loop: for each expert in order, every flat entry routed to it in order."""
    flat = [int(v) for v in np.asarray(indices).ravel()]
    perm, rev = [], [-1] * len(flat)
    counts = [0] * E
    for e in range(E):
        for f, v in enumerate(flat):
            if v == e:
                rev[f] = len(perm)
                perm.append(f)
                counts[e] += 1
    offsets = [0]
    for c in counts:
        offsets.append(offsets[-1] + c)
    perm += [-1] * (len(flat) - len(perm))
    return (np.array(counts, np.int32), np.array(offsets, np.int32), np.array(perm, np.int32), np.array(rev, np.int32))


def tile_table(offsets: np.ndarray, T: int, k: int, E: int) -> np.ndarray:
    """[ceil(T*k / 128) + E, 2]: {expert, first row} per 128-row piece of each non-empty segment, then {-1, 0}."""
    rows = []
    for e in range(E):
        for r in range(int(offsets[e]), int(offsets[e + 1]), TILE_ROWS):
            rows.append((e, r))
    n = -(-T * k // TILE_ROWS) + E
    rows += [(-1, 0)] * (n - len(rows))
    return np.array(rows, np.int32).reshape(n, 2)


def expand_offsets(offsets: np.ndarray, nrows: int) -> np.ndarray:
    E = len(offsets) - 1
    ids = np.full(nrows, -1, np.int32)
    for e in range(E):
        ids[offsets[e]:offsets[e + 1]] = e
    return ids


def scatter(y: np.ndarray, w: np.ndarray, rev: np.ndarray, k: int) -> np.ndarray:
    """fp32 sum in slot order (scatter_with_reverse_perm_kernel); y [T*k, H] fp32 values."""
    T = w.shape[0]
    out = np.zeros((T, y.shape[1]), np.float32)
    for s in range(k):
        r = rev.reshape(T, k)[:, s]
        ok = r >= 0
        term = np.where(ok[:, None], w[:, s:s + 1].astype(np.float32) * y[np.where(ok, r, 0)], np.float32(0.0))
        out = (out + term.astype(np.float32)).astype(np.float32)
    return out


def dequant_experts(codes: np.ndarray, scales_bits: np.ndarray) -> np.ndarray:
    """[E, N, K] codes + [E, N/128, K/128] bf16 bits -> fp32 lut[code] * float(scale), no bf16 rounding."""
    return np.stack([O.dequantize_fp8_e4m3_block(codes[e], scales_bits[e]) for e in range(codes.shape[0])])


def grouped_gemm(a: np.ndarray, w: np.ndarray, ids: np.ndarray) -> np.ndarray:
    """C[r] = a[r] . w[ids[r]]^T (fp32 result; rows whose id is outside [0, E) are zero)."""
    E = w.shape[0]
    out = np.zeros((a.shape[0], w.shape[1]), np.float64)
    for e in range(E):
        rows = np.nonzero(ids == e)[0]
        if rows.size:
            out[rows] = np.asarray(a[rows], np.float64) @ np.asarray(w[e], np.float64).T
    return out.astype(np.float32)


class RefMoE:
    """MoELayer on fp32 NumPy: router logits rounded to bf16 (the router is a bf16 Linear), top-k + softmax, then the
    k experts' SwiGLU MLPs and the weighted sum.  `gate` [E, H]; experts: list of (gate [I, H], up [I, H], down [H, I])
    fp32 weights (fp8 experts: dequant_experts values).  min_margin records the smallest top-k margin seen."""

    def __init__(self, gate: np.ndarray, experts, k: int):
        self.gate = np.asarray(gate, np.float32)
        self.experts = experts            # experts[e] -> (gate, up, down); may build them on demand
        self.k = k
        self.min_margin = float("inf")

    def __call__(self, x):
        x = np.asarray(x, np.float32)
        logits32 = x @ self.gate.T
        self.min_margin = min(self.min_margin, topk_margin(logits32, self.k))
        w, idx = topk_softmax(O.bf16_round(logits32), self.k, bf16=True)
        y = np.zeros((x.shape[0], self.k, x.shape[1]), np.float32)
        for e in np.unique(idx):
            t, s = np.nonzero(idx == e)
            g, u, d = (np.asarray(p, np.float32) for p in self.experts[int(e)])
            h = O.silu(x[t] @ g.T) * (x[t] @ u.T)
            y[t, s] = h @ d.T
        out = np.zeros_like(x)
        for s in range(self.k):
            out += w[:, s:s + 1] * y[:, s]
        return out
