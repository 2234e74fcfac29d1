"""Row normalisations (reference: src/pygpukit/ops/nn/norm.py:16-218 -> ops.cuh:143-155) and group normalisation
(csrc/ops_groupnorm.hip; the reference computes group_norm_silu's SiLU on the host)."""

from __future__ import annotations

from pygpukit_amd import _hip
from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import as_dtype
from pygpukit_amd.ops._common import call, check_out, validate_float, validate_same_dtype


def _check(input: GPUArray, gamma: GPUArray, name: str) -> None:
    validate_float(input, name)
    if input.ndim != 2:
        raise ValueError(f"{name} expects 2D input [batch, features], got {input.ndim}D")
    if gamma.ndim != 1:
        raise ValueError(f"{name} expects 1D gamma")
    validate_same_dtype(input, gamma, name)
    if input.shape[1] != gamma.shape[0]:
        raise ValueError(f"{name}: input features ({input.shape[1]}) must match gamma size ({gamma.shape[0]})")


def rmsnorm(input: GPUArray, gamma: GPUArray, eps: float = 1e-5, *, out: GPUArray | None = None) -> GPUArray:
    _check(input, gamma, "rmsnorm")
    o = check_out(out, input.shape, input.dtype, "rmsnorm")
    call("pgk_rmsnorm", input._p, gamma._p, o._p, input.shape[0], input.shape[1], eps, input.dtype.code, None)
    return o


def layernorm(input: GPUArray, gamma: GPUArray, beta: GPUArray, eps: float = 1e-5, *, out: GPUArray | None = None) -> GPUArray:
    _check(input, gamma, "layernorm")
    if beta.shape != gamma.shape or beta.dtype != gamma.dtype:
        raise ValueError("layernorm: beta must match gamma")
    o = check_out(out, input.shape, input.dtype, "layernorm")
    call("pgk_layernorm", input._p, gamma._p, beta._p, o._p, input.shape[0], input.shape[1], eps, input.dtype.code, None)
    return o


def _gn_dims(shape, channels_last: bool, name: str):
    if len(shape) != 4:
        raise ValueError(f"{name} expects 4D input [N, C, H, W] (or [N, H, W, C] with channels_last), got {len(shape)}D")
    if channels_last:
        n, h, w, c = shape
    else:
        n, c, h, w = shape
    if min(n, c, h, w) < 1:
        raise ValueError(f"{name}: input has an empty dimension, shape {tuple(shape)}")
    return n, c, h * w


def _gn_check_groups(n: int, c: int, hw: int, num_groups: int, name: str) -> None:
    if num_groups < 1 or c % num_groups:
        raise ValueError(f"{name}: channels ({c}) must be divisible by num_groups ({num_groups})")
    if n > 65535 or num_groups > 65535 or (c // num_groups) * hw >= 2 ** 31:
        raise ValueError(f"{name}: needs N <= 65535, num_groups <= 65535 and a group below 2^31 elements")


def group_norm_plan(n: int, c: int, hw: int, num_groups: int, dtype="float32", channels_last: bool = False) -> str:
    """"block" (one workgroup per image and group, one launch) or "split" (per-chunk partial statistics, then a fixed-order
    merge and the normalisation: two launches) for groups above 32768 elements.  PGK_GN_SPLIT=0/1 forces the plan.  Host logic."""
    _gn_check_groups(int(n), int(c), int(hw), int(num_groups), "group_norm_plan")
    plan = _hip.load().pgk_group_norm_plan(int(n), int(c), int(hw), int(num_groups), as_dtype(dtype).code, 1 if channels_last else 0)
    if plan < 0:
        raise ValueError(f"group_norm_plan: bad shape or dtype (N={n} C={c} HW={hw} groups={num_groups} {dtype})")
    return "split" if plan else "block"


def _group_norm(input, gamma, beta, num_groups, eps, channels_last, out, act, name):
    validate_float(input, name)
    n, c, hw = _gn_dims(input.shape, channels_last, name)
    if gamma.shape != (c,) or beta.shape != (c,):
        raise ValueError(f"{name}: gamma and beta must be [{c}], got {gamma.shape} and {beta.shape}")
    if gamma.dtype != input.dtype or beta.dtype != input.dtype:
        raise ValueError(f"{name}: gamma and beta must have the input's dtype {input.dtype}")
    _gn_check_groups(n, c, hw, int(num_groups), name)
    o = check_out(out, input.shape, input.dtype, name)
    call("pgk_group_norm", input._p, gamma._p, beta._p, o._p, n, c, hw, int(num_groups), float(eps), act, 1 if channels_last else 0,
         input.dtype.code, None)
    return o


def group_norm(input: GPUArray, gamma: GPUArray, beta: GPUArray, num_groups: int, eps: float = 1e-5, *, channels_last: bool = False,
               out: GPUArray | None = None) -> GPUArray:
    """input [N, C, H, W] (channels_last=True: [N, H, W, C]): every group of C / num_groups consecutive channels of an image is
    normalised by its own mean and population variance, then * gamma[c] + beta[c].  fp32 statistics (Welford / Chan), one
    rounding, run-to-run identical."""
    return _group_norm(input, gamma, beta, num_groups, eps, channels_last, out, 0, "group_norm")


def group_norm_silu(input: GPUArray, gamma: GPUArray, beta: GPUArray, num_groups: int, eps: float = 1e-5, *,
                    channels_last: bool = False, out: GPUArray | None = None) -> GPUArray:
    """silu(group_norm(...)) in the same launch: the SiLU is applied to the fp32 value before the one rounding."""
    return _group_norm(input, gamma, beta, num_groups, eps, channels_last, out, 1, "group_norm_silu")
