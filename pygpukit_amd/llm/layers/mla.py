"""[build-defined] Multi-head latent attention layer (DeepSeek-V2 / V3 / R1, Kimi-K2) over a fixed latent cache, absorbed form.

Constructed from the HF-named weights, RoPE rows already in this project's half layout:
  q_proj [H * (nope + 64), hidden]   or   q_a_proj [q_lora, hidden] / q_a_layernorm [q_lora] / q_b_proj [H * (nope + 64), q_lora]
  kv_a_proj_with_mqa [512 + 64, hidden], kv_a_layernorm [512], kv_b_proj [H * (nope + v), 512], o_proj [hidden, H * v]
At load kv_b_proj is split once, on the device, into W_UK [H, nope, 512] and W_UV [H, v, 512] (and W_UV^T [H, 512, v], the operand of
the output GEMM), and the query projection's rows into the heads' no-position rows and their rope rows, so both come out contiguous.

forward_fixed_cache(x [S, hidden], start_position): the query projections; q_abs = q_nope . W_UK per head (batched_matmul) and
rope_inplace on q_pe; ONE SMALL PACK of both into the [S, H, 576] query buffer (transposes and a row concatenation of existing ops: no
op here writes a strided output); mla_cache_write; sdpa_mla_fixed_cache; o = out . W_UV^T per head; o_proj.  Only existing ops run
around the two new ones.  Out of scope: INTEGRATION.md.

forward_prefill(x, start_position), at nope = v = 128: the same chunk in the decompressed form - one GEMM with the unsplit kv_b_proj over
the latent rows, then sdpa_mla_prefill (ops_mla_prefill.hip), 3.4 times less attention arithmetic and no per-head matmul, transpose or
pack.  Both methods write the same cache rows, so prompts go through forward_prefill and decode steps through forward_fixed_cache.

forward_paged(x [num_seqs, hidden], positions, slot_mapping, block_tables, context_lens, cache, max_context): one decode token per
sequence of a batch over a PAGED latent cache the caller owns - mla_reshape_and_cache and sdpa_mla_paged (ops_mla_paged.hip) in the
places of the two ops above, every length on the device."""

from __future__ import annotations

import numpy as np

from pygpukit_amd import _hip
from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import int32
from pygpukit_amd.core.factory import from_numpy, zeros
from pygpukit_amd.ops.matmul import batched_matmul, transpose
from pygpukit_amd.ops.nn.linear import split_qkv_batch
from pygpukit_amd.ops.nn.mla import (LATENT, PREFILL_NOPE, PREFILL_V, ROPE, WIDTH, mla_cache_write, mla_reshape_and_cache, sdpa_mla_fixed_cache,
                                     sdpa_mla_paged, sdpa_mla_prefill)
from pygpukit_amd.ops.nn.norm import rmsnorm
from pygpukit_amd.ops.nn.rope import rope_inplace_f32table
from pygpukit_amd.ops.paged import gather_embeddings
from pygpukit_amd.ops.tensor import concat_axis0, transpose_3d_012, transpose_3d_021

from .linear import LinearBF16
from .rope import precompute_freqs_cis


def _gather_rows(src: GPUArray, dst: GPUArray, heads: int, src_head_rows: int, first: int, count: int) -> None:
    """dst [heads * count, cols] <- rows first .. first + count - 1 of each head's src_head_rows rows of src: one device copy per head."""
    row = src.shape[-1] * src.itemsize
    for h in range(heads):
        _hip.call("pgk_memcpy_d2d", dst.data_ptr() + h * count * row, src.data_ptr() + (h * src_head_rows + first) * row, count * row, None)


class MLAttention:
    def __init__(self, *, num_heads: int, qk_nope_head_dim: int, v_head_dim: int, softmax_scale: float, kv_a_proj_with_mqa: GPUArray,
                 kv_a_layernorm: GPUArray, kv_b_proj: GPUArray, o_proj: GPUArray, q_proj: GPUArray | None = None,
                 q_a_proj: GPUArray | None = None, q_a_layernorm: GPUArray | None = None, q_b_proj: GPUArray | None = None,
                 qk_rope_head_dim: int = ROPE, kv_lora_rank: int = LATENT, max_position_embeddings: int = 4096, rope_theta: float = 10000.0,
                 norm_eps: float = 1e-6):
        if qk_rope_head_dim != ROPE or kv_lora_rank != LATENT:
            raise ValueError(f"MLAttention: qk_rope_head_dim must be {ROPE} and kv_lora_rank {LATENT} (the latent cache row is {WIDTH} wide)")
        if (q_proj is None) == (q_a_proj is None) or (q_a_proj is not None and (q_a_layernorm is None or q_b_proj is None)):
            raise ValueError("MLAttention: give q_proj, or q_a_proj with q_a_layernorm and q_b_proj")
        if not softmax_scale > 0:
            raise ValueError(f"MLAttention: softmax_scale must be positive, got {softmax_scale}")
        H, nope, v = num_heads, qk_nope_head_dim, v_head_dim
        qw = q_proj if q_proj is not None else q_b_proj
        if qw.shape[0] != H * (nope + ROPE) or kv_a_proj_with_mqa.shape[0] != WIDTH or kv_b_proj.shape != (H * (nope + v), LATENT) \
                or o_proj.shape[1] != H * v or kv_a_layernorm.shape != (LATENT,):
            raise ValueError("MLAttention: weight shapes do not match num_heads / qk_nope_head_dim / v_head_dim")
        self.num_heads, self.qk_nope_head_dim, self.v_head_dim, self.softmax_scale, self.norm_eps = H, nope, v, float(softmax_scale), norm_eps
        self.q_a_proj = LinearBF16(q_a_proj) if q_a_proj is not None else None
        self.q_a_layernorm = q_a_layernorm
        # the query projection's rows, regrouped: every head's no-position rows, then every head's rope rows
        q_nope_w, q_pe_w = GPUArray((H * nope, qw.shape[1]), qw.dtype), GPUArray((H * ROPE, qw.shape[1]), qw.dtype)
        _gather_rows(qw, q_nope_w, H, nope + ROPE, 0, nope)
        _gather_rows(qw, q_pe_w, H, nope + ROPE, nope, ROPE)
        self.q_nope_proj, self.q_pe_proj = LinearBF16(q_nope_w), LinearBF16(q_pe_w)
        self.kv_a_proj_with_mqa, self.kv_a_layernorm, self.o_proj = LinearBF16(kv_a_proj_with_mqa), kv_a_layernorm, LinearBF16(o_proj)
        self.w_uk, self.w_uv = GPUArray((H, nope, LATENT), kv_b_proj.dtype), GPUArray((H, v, LATENT), kv_b_proj.dtype)
        _gather_rows(kv_b_proj, self.w_uk, H, nope + v, 0, nope)
        _gather_rows(kv_b_proj, self.w_uv, H, nope + v, nope, v)
        self._w_uv_t = transpose_3d_012(self.w_uv)          # W_UV^T per head [H, 512, v]: the [K, N] operand of out . W_UV^T
        self.kv_b_proj = LinearBF16(kv_b_proj)              # unsplit, forward_prefill's decompression GEMM
        cos, sin = precompute_freqs_cis(ROPE, max_position_embeddings, rope_theta)
        self._cos, self._sin = from_numpy(cos.astype(np.float32)), from_numpy(sin.astype(np.float32))
        self._cache: GPUArray | None = None

    def init_fixed_cache(self, max_seq: int, dtype: str = "bfloat16") -> None:
        """One latent cache [max_seq, 576] for all heads."""
        if max_seq > self._cos.shape[0]:
            raise ValueError(f"init_fixed_cache: {max_seq} rows beyond max_position_embeddings {self._cos.shape[0]}")
        self._cache = zeros((max_seq, WIDTH), dtype)

    def forward_fixed_cache(self, x: GPUArray, start_position: int) -> GPUArray:
        """x [S, hidden], a prompt chunk or one token at positions start_position ..: writes their latent rows, attends rows
        0 .. start_position + S - 1, returns [S, hidden]."""
        if self._cache is None:
            raise RuntimeError("MLAttention: init_fixed_cache first")
        S, H = x.shape[0], self.num_heads
        if start_position < 0 or start_position + S > self._cache.shape[0]:
            raise ValueError(f"forward_fixed_cache: positions {start_position}..{start_position + S - 1} outside the cache of {self._cache.shape[0]} rows")
        cos, sin = self._cos._view(start_position * ROPE, (S, ROPE)), self._sin._view(start_position * ROPE, (S, ROPE))
        q = self._absorbed_query(x, cos, sin)
        mla_cache_write(self.kv_a_proj_with_mqa(x), self.kv_a_layernorm, self._cos, self._sin, self._cache, start_position, self.norm_eps)
        out = GPUArray((S, H, LATENT), x.dtype)
        sdpa_mla_fixed_cache(q, self._cache, out, start_position + S, self.softmax_scale)
        return self._project_out(out)

    def _absorbed_query(self, x: GPUArray, cos: GPUArray, sin: GPUArray) -> GPUArray:
        """x [S, hidden], cos / sin [S, 64] (row s: token s's position) -> q [S, H, 576] = [q_nope . W_UK | RoPE(q_pe)]."""
        S, H, nope = x.shape[0], self.num_heads, self.qk_nope_head_dim
        xq = x if self.q_a_proj is None else rmsnorm(self.q_a_proj(x), self.q_a_layernorm, self.norm_eps)
        q_nope = self.q_nope_proj(xq).view((S, H, nope))
        q_pe = self.q_pe_proj(xq).view((S, H, ROPE))
        rope_inplace_f32table(q_pe, q_pe._view(0, (S, 0, ROPE)), cos, sin)
        # [S, H, *] and [H, S, *] are the same bytes for one token
        q_nope_h = q_nope.view((H, 1, nope)) if S == 1 else transpose_3d_021(q_nope)
        q_abs = batched_matmul(q_nope_h, self.w_uk)                                  # [H, S, 512]
        q_abs = q_abs.view((H * S, LATENT)) if S == 1 else transpose_3d_021(q_abs).view((S * H, LATENT))
        # the pack: [q_abs | q_pe] per (row, head) = rows of [576, S H] concatenated, transposed back
        return transpose(concat_axis0(transpose(q_abs), transpose(q_pe.view((S * H, ROPE))))).view((S, H, WIDTH))

    def _project_out(self, out: GPUArray) -> GPUArray:
        """The attention's latent output [S, H, 512] -> o = out . W_UV^T per head -> o_proj -> [S, hidden]."""
        S, H, v = out.shape[0], self.num_heads, self.v_head_dim
        out_h = out.view((H, 1, LATENT)) if S == 1 else transpose_3d_021(out)
        o = batched_matmul(out_h, self._w_uv_t)                                      # [H, S, v]
        o = o.view((1, H * v)) if S == 1 else transpose_3d_021(o).view((S, H * v))
        return self.o_proj(o)

    def forward_paged(self, x: GPUArray, positions: GPUArray, slot_mapping: GPUArray, block_tables: GPUArray, context_lens: GPUArray,
                      cache: GPUArray, max_context: int) -> GPUArray:
        """One decode token per sequence of a batch over a paged latent cache (ops.nn.allocate_mla_cache): x [num_seqs, hidden],
        positions / slot_mapping / context_lens int32 [num_seqs] on the device (context_lens counts this token), block_tables int32
        [num_seqs, max_blocks_per_seq], max_context the host's bound on context_lens.  The query projections with RoPE at each
        sequence's own position (the table rows gathered by position), mla_reshape_and_cache, the absorbed query, sdpa_mla_paged,
        W_UV and o_proj: row b is what forward_fixed_cache returns for sequence b alone.  No length is read on the host, so positions must
        lie below max_position_embeddings: they index the RoPE tables."""
        n, H = x.shape[0], self.num_heads
        if positions.dtype != int32 or positions.ndim != 1 or positions.shape[0] != n:
            raise ValueError(f"forward_paged: positions must be int32 [{n}], got {positions.shape}/{positions.dtype}")
        cos, sin = gather_embeddings(positions, self._cos, n), gather_embeddings(positions, self._sin, n)
        q = self._absorbed_query(x, cos, sin)
        mla_reshape_and_cache(self.kv_a_proj_with_mqa(x), self.kv_a_layernorm, self._cos, self._sin, positions, cache, slot_mapping, self.norm_eps)
        out = GPUArray((n, 1, H, LATENT), x.dtype)
        sdpa_mla_paged(q.view((n, 1, H, WIDTH)), cache, block_tables, context_lens, out, max_context, self.softmax_scale)
        return self._project_out(out.view((n, H, LATENT)))

    def forward_prefill(self, x: GPUArray, start_position: int) -> GPUArray:
        """forward_fixed_cache for a prompt chunk in the decompressed form (qk_nope_head_dim = v_head_dim = 128 only): the query
        projections and RoPE; mla_cache_write; the latent columns of cache rows 0 .. T - 1 (T = start_position + S) split off into a
        contiguous [T, 512]; ONE GEMM with the unsplit kv_b_proj -> kv [T, H * 256]; sdpa_mla_prefill; o_proj.  No per-head matmul,
        transpose or pack.  Decode steps continue through forward_fixed_cache on the same cache.  The decompression GEMM covers the
        whole prefix at every chunk, so a short chunk over a long prefix belongs to forward_fixed_cache."""
        H, nope, v = self.num_heads, self.qk_nope_head_dim, self.v_head_dim
        if nope != PREFILL_NOPE or v != PREFILL_V:
            raise ValueError(f"forward_prefill: needs qk_nope_head_dim = {PREFILL_NOPE} and v_head_dim = {PREFILL_V}, got {nope} and {v}")
        if self._cache is None:
            raise RuntimeError("MLAttention: init_fixed_cache first")
        S, T = x.shape[0], start_position + x.shape[0]
        if start_position < 0 or T > self._cache.shape[0]:
            raise ValueError(f"forward_prefill: positions {start_position}..{T - 1} outside the cache of {self._cache.shape[0]} rows")
        xq = x if self.q_a_proj is None else rmsnorm(self.q_a_proj(x), self.q_a_layernorm, self.norm_eps)
        q_nope = self.q_nope_proj(xq).view((S, H, nope))
        q_pe = self.q_pe_proj(xq).view((S, H, ROPE))
        cos, sin = self._cos._view(start_position * ROPE, (S, ROPE)), self._sin._view(start_position * ROPE, (S, ROPE))
        rope_inplace_f32table(q_pe, q_pe._view(0, (S, 0, ROPE)), cos, sin)
        mla_cache_write(self.kv_a_proj_with_mqa(x), self.kv_a_layernorm, self._cos, self._sin, self._cache, start_position, self.norm_eps)
        latent, kpe_lo, kpe_hi = GPUArray((T, LATENT), x.dtype), GPUArray((T, ROPE // 2), x.dtype), GPUArray((T, ROPE // 2), x.dtype)
        split_qkv_batch(self._cache._view(0, (T, WIDTH)), latent, kpe_lo, kpe_hi, LATENT, ROPE // 2, ROPE // 2)
        kv = self.kv_b_proj(latent).view((T, H, nope + v))
        out = GPUArray((S, H, v), x.dtype)
        sdpa_mla_prefill(q_nope, q_pe, kv, self._cache, out, T, self.softmax_scale)
        return self.o_proj(out.view((S, H * v)))


__all__ = ["MLAttention"]
