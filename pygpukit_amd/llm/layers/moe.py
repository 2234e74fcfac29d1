"""Mixture-of-Experts feed-forward layer (reference: src/pygpukit/llm/layers/moe.py), for Mixtral and Qwen3-MoE.

forward: router GEMM -> fused top-k + softmax -> stable permutation -> grouped gate|up GEMM (rows read through the
permutation, no gathered copy) -> SwiGLU -> grouped down GEMM (fp32 split-K slabs) -> weighted scatter.  Every launch is
sized from the token count alone: no host synchronisation and no per-expert Python loop, so a forward can be captured
into a graph and replayed with tokens that route differently.  The experts are stacked once here: gate and up as one
[E, 2I, H] weight, down as [E, H, I] (bf16, or fp8 codes with their 128x128 block scales)."""

from __future__ import annotations

from typing import TYPE_CHECKING

from pygpukit_amd import _hip
from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import bfloat16, int32, uint8
from pygpukit_amd.ops.matmul.grouped import grouped_gemm_bf16, grouped_gemm_fp8_bf16
from pygpukit_amd.ops.moe import moe_compute_permutation, moe_scatter, moe_topk_softmax
from pygpukit_amd.ops.nn.fused import glu_packed

from .linear import LinearBF16, LinearFP8

if TYPE_CHECKING:
    from pygpukit_amd.llm.config import TransformerConfig


def _stack(parts: list[list[GPUArray]], dtype) -> GPUArray:
    """parts[e] = arrays concatenated along their first axis into expert e's slice of one [E, rows, cols] array."""
    rows = sum(p.shape[0] for p in parts[0])
    cols = parts[0][0].shape[1]
    out = GPUArray((len(parts), rows, cols), dtype)
    off = 0
    for group in parts:
        for p in group:
            if p.dtype != dtype or p.ndim != 2 or p.shape[1] != cols:
                raise ValueError(f"MoELayer: expert weights must share dtype {dtype} and width {cols}, got {p.dtype} {p.shape}")
            _hip.call("pgk_memcpy_d2d", GPUArray._view(out, off, p.shape)._p, p._p, p.nbytes, None)
            off += p.size
    if off != out.size:
        raise ValueError("MoELayer: experts differ in shape")
    return out


class MoELayer:
    """MoELayer(config, gate_weight [E, H], expert_weights [(gate, up, down), ...]); each projection a bf16 GPUArray
    [out, in], a LinearBF16 or a LinearFP8.  Called on x [T, H] or [B, S, H]."""

    # what the model's zero-allocation MLP path and the decode strategies look at: they take their generic branch
    activation = "silu"
    gate_up_proj = None

    def __init__(self, config: "TransformerConfig", gate_weight: GPUArray, expert_weights: list):
        self.config = config
        self.num_experts = config.num_experts or len(expert_weights)
        self.num_experts_per_tok = config.num_experts_per_tok
        self.hidden_size = config.hidden_size
        self.intermediate_size = config.moe_intermediate_size or config.intermediate_size
        if len(expert_weights) != self.num_experts:
            raise ValueError(f"MoELayer: {len(expert_weights)} experts given, config says {self.num_experts}")
        self.gate = LinearBF16(gate_weight)
        first = expert_weights[0][0]
        self.fp8 = isinstance(first, LinearFP8)
        if self.fp8:
            if not all(isinstance(p, LinearFP8) for ew in expert_weights for p in ew):
                raise ValueError("MoELayer: fp8 experts must all be LinearFP8")
            self.w_gate_up = _stack([[g.weight_fp8, u.weight_fp8] for g, u, _ in expert_weights], uint8)
            self.s_gate_up = _stack([[g.scale_inv, u.scale_inv] for g, u, _ in expert_weights], bfloat16)
            self.w_down = _stack([[d.weight_fp8] for _, _, d in expert_weights], uint8)
            self.s_down = _stack([[d.scale_inv] for _, _, d in expert_weights], bfloat16)
        else:
            def w(p):
                if isinstance(p, LinearBF16):
                    if p.bias is not None:
                        raise ValueError("MoELayer: expert projections have no bias")
                    return p.weight
                if isinstance(p, GPUArray):
                    return p
                raise ValueError(f"MoELayer: unsupported expert weight {type(p).__name__}")
            self.w_gate_up = _stack([[w(g), w(u)] for g, u, _ in expert_weights], bfloat16)
            self.w_down = _stack([[w(d)] for _, _, d in expert_weights], bfloat16)
            self.s_gate_up = self.s_down = None
        E, I, H = self.num_experts, self.intermediate_size, self.hidden_size
        if self.w_gate_up.shape != (E, 2 * I, H) or self.w_down.shape != (E, H, I):
            raise ValueError(f"MoELayer: stacked experts {self.w_gate_up.shape} / {self.w_down.shape} do not match "
                             f"E={E}, I={I}, H={H}")
        if gate_weight.shape != (E, H):
            raise ValueError(f"MoELayer: router weight {gate_weight.shape} != ({E}, {H})")

    def _grouped(self, a, w, s, **kw):
        if self.fp8:
            return grouped_gemm_fp8_bf16(a, w, s, None, **kw)
        return grouped_gemm_bf16(a, w, None, **kw)

    def __call__(self, x: GPUArray) -> GPUArray:
        shape = x.shape
        if x.ndim == 3:
            x = x.reshape(shape[0] * shape[1], shape[2])
        elif x.ndim != 2:
            raise ValueError(f"MoELayer: input must be [T, H] or [B, S, H], got {shape}")
        if x.shape[1] != self.hidden_size or x.dtype != bfloat16:
            raise ValueError(f"MoELayer: input must be bfloat16 [T, {self.hidden_size}], got {x.dtype} {x.shape}")
        T, E, k, I = x.shape[0], self.num_experts, self.num_experts_per_tok, self.intermediate_size

        logits = self.gate(x)                                                     # [T, E]
        weights, indices = GPUArray((T, k), logits.dtype), GPUArray((T, k), int32)
        moe_topk_softmax(logits, weights, indices, k)
        counts, offsets = GPUArray((E,), int32), GPUArray((E + 1,), int32)
        perm, rperm = GPUArray((T * k,), int32), GPUArray((T * k,), int32)
        tiles = moe_compute_permutation(indices, counts, offsets, perm, rperm, E, k)

        gate_up = self._grouped(x, self.w_gate_up, self.s_gate_up, tiles=tiles, expert_offsets=offsets,
                                permute_indices=perm, top_k=k)                    # [T*k, 2I], sorted rows
        act = glu_packed(gate_up, I)
        # act is already in sorted order: T*k rows with k = 1 give the same tile table, regime and K splits
        slabs = self._grouped(act, self.w_down, self.s_down, tiles=tiles, expert_offsets=offsets, out_slabs=True)
        out = GPUArray((T, self.hidden_size), x.dtype)
        moe_scatter(slabs, weights, rperm, out, k)
        return out.reshape(*shape) if len(shape) == 3 else out
