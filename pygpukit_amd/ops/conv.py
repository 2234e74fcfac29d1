"""conv1d and conv2d (reference: src/pygpukit/ops/conv.py -> native/ops/conv/conv1d_kernels.cuh, conv2d_kernels.cuh).

    out[b, m, n] = bias[m] + sum_{c, t} weight[m, c, t] * input[b, c, n * stride + t - padding]      zeros outside [0, L)

bfloat16 / float16 run an implicit GEMM on the 32x32x16 MFMA (csrc/ops_conv.hip), float32 a tiled FMA kernel, which is also
the general path for the 16-bit calls the MFMA kernel declines (conv1d_plan).  The keyword-only arguments are
[build-defined]; their defaults reproduce the reference.  Contract: INTEGRATION.md.

conv2d is the same pair of kernels in two dimensions (csrc/ops_conv2d.hip):

    out[n, m, oy, ox] = bias[m] + sum_{c, ky, kx} weight[m, c, ky, kx] * X[n, c, oy*sh + ky*dh - ph, ox*sw + kx*dw - pw]

with zeros outside X, and X the input or (upsample=2) its nearest-neighbour 2x, read through (y >> 1, x >> 1)."""

from __future__ import annotations

from pygpukit_amd import _hip
from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import DataType, as_dtype, float32
from pygpukit_amd.ops._common import call, check_out, validate_float

_ACTIVATIONS = {None: 0, "gelu": 1}


def _out_length(c_in: int, c_out: int, length: int, k: int, stride: int, padding: int, name: str) -> int:
    if min(c_in, c_out, length, k) < 1:
        raise ValueError(f"{name}: C_in, C_out, L and K must be >= 1, got C_in={c_in} C_out={c_out} L={length} K={k}")
    if stride < 1 or padding < 0:
        raise ValueError(f"{name}: needs stride >= 1 and padding >= 0, got stride={stride} padding={padding}")
    l_out = (length + 2 * padding - k) // stride + 1
    if length + 2 * padding < k or l_out < 1:
        raise ValueError(f"{name}: L_out < 1 for L={length} K={k} stride={stride} padding={padding}")
    if length + 2 * padding >= 2 ** 31:
        raise ValueError(f"{name}: L + 2 * padding must stay below 2^31")
    return l_out


def conv1d_plan(in_channels: int, out_channels: int, length: int, kernel_size: int, stride: int = 1, padding: int = 0,
                dtype: "str | DataType" = float32) -> str:
    """Which kernel a call of this shape takes under the current environment: "mfma" or "fma" (PGK_CONV_MFMA=0 forces
    "fma").  Host logic only, needs no device.  A caller's misaligned packed_weight also falls to "fma"."""
    dt = as_dtype(dtype)
    _out_length(int(in_channels), int(out_channels), int(length), int(kernel_size), int(stride), int(padding), "conv1d_plan")
    plan = _hip.load().pgk_conv1d_plan(int(in_channels), int(out_channels), int(length), int(kernel_size), int(stride), int(padding), dt.code)
    if plan < 0:
        raise ValueError(f"conv1d_plan requires float32/float16/bfloat16, got {dt}")
    return "mfma" if plan else "fma"


def conv1d_pack_weight(weight: GPUArray) -> GPUArray:
    """[build-defined] weight [C_out, C_in, K] (bfloat16 / float16) -> the image the MFMA kernel reads,
    [K, C_out padded to 64, C_in padded to 32] with zeros in the padding.  Pass it as conv1d(..., packed_weight=) so a model
    packs once instead of once per call."""
    if weight.ndim != 3 or 0 in weight.shape:
        raise ValueError(f"conv1d_pack_weight: weight must be 3D [out_channels, in_channels, kernel_size], got shape {weight.shape}")
    validate_float(weight, "conv1d_pack_weight: weight")
    if weight.dtype == float32:
        raise ValueError("conv1d_pack_weight: weight must be float16/bfloat16 (the float32 kernel reads the weight as it is)")
    c_out, c_in, k = weight.shape
    packed = GPUArray((k, -(-c_out // 64) * 64, -(-c_in // 32) * 32), weight.dtype)
    assert packed.size == _hip.load().pgk_conv1d_packed_elems(c_in, c_out, k)
    call("pgk_conv1d_pack_weight", weight._p, packed._p, c_in, c_out, k, weight.dtype.code, None)
    return packed


def conv1d(input: GPUArray, weight: GPUArray, bias: GPUArray | None = None, stride: int = 1, padding: int = 0, *,
           activation: str | None = None, channels_last_out: bool = False, add: GPUArray | None = None,
           packed_weight: GPUArray | None = None, out: GPUArray | None = None) -> GPUArray:
    """input [B, C_in, L], weight [C_out, C_in, K], bias [C_out] or None -> [B, C_out, L_out],
    L_out = (L + 2 * padding - K) // stride + 1, zero padding.

    activation="gelu": the tanh GELU on the fp32 accumulator after the bias.  channels_last_out=True: the result is written
    as [B, L_out, C_out].  add: [L_out, C_out] of the same dtype, added after the activation to every batch element (only with
    channels_last_out).  packed_weight: conv1d_pack_weight(weight).  Everything is rounded once, on the store."""
    if input.ndim != 3:
        raise ValueError(f"conv1d: input must be 3D [batch, in_channels, length], got {input.ndim}D")
    if weight.ndim != 3:
        raise ValueError(f"conv1d: weight must be 3D [out_channels, in_channels, kernel_size], got {weight.ndim}D")
    validate_float(input, "conv1d: input")
    batch, c_in, length = input.shape
    c_out, wc_in, k = weight.shape
    if wc_in != c_in:
        raise ValueError(f"conv1d: weight in_channels {wc_in} does not match input in_channels {c_in}")
    if batch < 1:
        raise ValueError(f"conv1d: input has an empty dimension, shape {input.shape}")
    l_out = _out_length(c_in, c_out, length, k, int(stride), int(padding), "conv1d")
    if weight.dtype != input.dtype:
        raise ValueError(f"conv1d: weight has dtype {weight.dtype}, input has {input.dtype}")
    if bias is not None and (bias.shape != (c_out,) or bias.dtype != input.dtype):
        raise ValueError(f"conv1d: bias must be [{c_out}] of dtype {input.dtype}, got {bias.shape} {bias.dtype}")
    if activation not in _ACTIVATIONS:
        raise ValueError(f"conv1d: activation must be None or 'gelu', got {activation!r}")
    if add is not None:
        if not channels_last_out:
            raise ValueError("conv1d: add needs channels_last_out=True")
        if add.shape != (l_out, c_out) or add.dtype != input.dtype:
            raise ValueError(f"conv1d: add must be [{l_out}, {c_out}] of dtype {input.dtype}, got {add.shape} {add.dtype}")
    if packed_weight is not None:
        want = (k, -(-c_out // 64) * 64, -(-c_in // 32) * 32)
        if packed_weight.shape != want or packed_weight.dtype != input.dtype or input.dtype == float32:
            raise ValueError(f"conv1d: packed_weight must be conv1d_pack_weight(weight): {want} of a 16-bit input dtype, got "
                             f"{packed_weight.shape} {packed_weight.dtype}")
    if batch > 65535:
        raise ValueError(f"conv1d: batch {batch} > 65535")
    o = check_out(out, (batch, l_out, c_out) if channels_last_out else (batch, c_out, l_out), input.dtype, "conv1d")
    call("pgk_conv1d", input._p, weight._p, packed_weight._p if packed_weight is not None else None,
         bias._p if bias is not None else None, add._p if add is not None else None, o._p, batch, c_in, c_out, length, k, int(stride),
         int(padding), _ACTIVATIONS[activation], 1 if channels_last_out else 0, input.dtype.code, None)
    return o


def _pair(v, name: str) -> "tuple[int, int]":
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"{name} must be an int or a pair, got {v!r}")
        return int(v[0]), int(v[1])
    return int(v), int(v)


def _out_size2d(c_in, c_out, h, w, kh, kw, stride, padding, dilation, upsample, name: str) -> "tuple[int, int]":
    (sh, sw), (ph, pw), (dh, dw) = stride, padding, dilation
    if min(c_in, c_out, h, w, kh, kw) < 1:
        raise ValueError(f"{name}: C_in, C_out, H, W, KH and KW must be >= 1, got C_in={c_in} C_out={c_out} H={h} W={w} K={kh}x{kw}")
    if min(sh, sw, dh, dw) < 1 or min(ph, pw) < 0:
        raise ValueError(f"{name}: needs stride >= 1, dilation >= 1 and padding >= 0, got stride={stride} padding={padding} dilation={dilation}")
    if upsample not in (1, 2):
        raise ValueError(f"{name}: upsample must be 1 or 2, got {upsample!r}")
    he, we = h * upsample + 2 * ph, w * upsample + 2 * pw
    if max(he, we) >= 2 ** 30:
        raise ValueError(f"{name}: H and W with upsample and padding must stay below 2^30")
    eh, ew = (kh - 1) * dh + 1, (kw - 1) * dw + 1
    if he < eh or we < ew:
        raise ValueError(f"{name}: output is empty for H={h} W={w} K={kh}x{kw} padding={padding} dilation={dilation}")
    return (he - eh) // sh + 1, (we - ew) // sw + 1


def conv2d_plan(in_channels: int, out_channels: int, height: int, width: int, kernel_size, stride=1, padding=0, dilation=1,
                dtype: "str | DataType" = float32, *, upsample: int = 1) -> str:
    """Which kernel a call of this shape takes under the current environment: "mfma" for bfloat16 / float16 with a square
    kernel of 1 or 3, equal strides of 1 or 2 and dilation 1; "fma" for float32 and everything else (PGK_CONV_MFMA=0 forces
    "fma").  Host logic only, needs no device.  A caller's misaligned packed_weight also falls to "fma"."""
    dt = as_dtype(dtype)
    k, s, p, d = _pair(kernel_size, "kernel_size"), _pair(stride, "stride"), _pair(padding, "padding"), _pair(dilation, "dilation")
    _out_size2d(int(in_channels), int(out_channels), int(height), int(width), k[0], k[1], s, p, d, upsample, "conv2d_plan")
    plan = _hip.load().pgk_conv2d_plan(int(in_channels), int(out_channels), int(height), int(width), k[0], k[1], s[0], s[1], p[0], p[1],
                                       d[0], d[1], int(upsample), dt.code)
    if plan < 0:
        raise ValueError(f"conv2d_plan requires float32/float16/bfloat16, got {dt}")
    return "mfma" if plan else "fma"


def _packed_shape2d(c_out: int, c_in: int, kh: int, kw: int) -> "tuple[int, int, int]":
    return kh * kw, -(-c_out // 64) * 64, -(-c_in // 32) * 32


def conv2d_pack_weight(weight: GPUArray) -> GPUArray:
    """[build-defined] weight [C_out, C_in, KH, KW] (bfloat16 / float16) -> the image the MFMA kernel reads,
    [KH * KW, C_out padded to 64, C_in padded to 32] with zeros in the padding; pass it as conv2d(..., packed_weight=)."""
    if weight.ndim != 4 or 0 in weight.shape:
        raise ValueError(f"conv2d_pack_weight: weight must be 4D [out_channels, in_channels, kh, kw], got shape {weight.shape}")
    validate_float(weight, "conv2d_pack_weight: weight")
    if weight.dtype == float32:
        raise ValueError("conv2d_pack_weight: weight must be float16/bfloat16 (the float32 kernel reads the weight as it is)")
    c_out, c_in, kh, kw = weight.shape
    packed = GPUArray(_packed_shape2d(c_out, c_in, kh, kw), weight.dtype)
    assert packed.size == _hip.load().pgk_conv2d_packed_elems(c_in, c_out, kh, kw)
    call("pgk_conv2d_pack_weight", weight._p, packed._p, c_in, c_out, kh, kw, weight.dtype.code, None)
    return packed


def conv2d(input: GPUArray, weight: GPUArray, bias: GPUArray | None = None, stride=1, padding=0, dilation=1, groups: int = 1, *,
           channels_last: bool = False, channels_last_out: bool = False, upsample: int = 1, add: GPUArray | None = None,
           packed_weight: GPUArray | None = None, out: GPUArray | None = None) -> GPUArray:
    """input [N, C_in, H, W], weight [C_out, C_in, KH, KW], bias [C_out] or None -> [N, C_out, H_out, W_out]; stride, padding and
    dilation are an int or a (h, w) pair; zero padding.  groups != 1 raises NotImplementedError.

    channels_last=True: the input is [N, H, W, C_in].  channels_last_out=True: the result is [N, H_out, W_out, C_out].
    upsample=2: the convolution reads the nearest-neighbour 2x of the input (never materialised).  add: an array of the
    output's shape, layout and dtype, added in fp32 after the bias.  packed_weight: conv2d_pack_weight(weight).  Everything is
    rounded once, on the store; all of it is one launch."""
    if groups != 1:
        raise NotImplementedError(f"conv2d: groups={groups} is not built (grouped convolution is out of scope)")
    if input.ndim != 4:
        raise ValueError(f"conv2d: input must be 4D [batch, in_channels, height, width], got {input.ndim}D")
    if weight.ndim != 4:
        raise ValueError(f"conv2d: weight must be 4D [out_channels, in_channels, kh, kw], got {weight.ndim}D")
    validate_float(input, "conv2d: input")
    if channels_last:
        batch, h, w, c_in = input.shape
    else:
        batch, c_in, h, w = input.shape
    c_out, wc_in, kh, kw = weight.shape
    if wc_in != c_in:
        raise ValueError(f"conv2d: weight in_channels {wc_in} does not match input in_channels {c_in}")
    if batch < 1:
        raise ValueError(f"conv2d: input has an empty dimension, shape {input.shape}")
    s, p, d = _pair(stride, "conv2d: stride"), _pair(padding, "conv2d: padding"), _pair(dilation, "conv2d: dilation")
    h_out, w_out = _out_size2d(c_in, c_out, h, w, kh, kw, s, p, d, upsample, "conv2d")
    if weight.dtype != input.dtype:
        raise ValueError(f"conv2d: weight has dtype {weight.dtype}, input has {input.dtype}")
    if bias is not None and (bias.shape != (c_out,) or bias.dtype != input.dtype):
        raise ValueError(f"conv2d: bias must be [{c_out}] of dtype {input.dtype}, got {bias.shape} {bias.dtype}")
    oshape = (batch, h_out, w_out, c_out) if channels_last_out else (batch, c_out, h_out, w_out)
    if add is not None and (add.shape != oshape or add.dtype != input.dtype):
        raise ValueError(f"conv2d: add must be {oshape} of dtype {input.dtype}, got {add.shape} {add.dtype}")
    if packed_weight is not None:
        want = _packed_shape2d(c_out, c_in, kh, kw)
        if packed_weight.shape != want or packed_weight.dtype != input.dtype or input.dtype == float32:
            raise ValueError(f"conv2d: packed_weight must be conv2d_pack_weight(weight): {want} of a 16-bit input dtype, got "
                             f"{packed_weight.shape} {packed_weight.dtype}")
    if batch > 65535:
        raise ValueError(f"conv2d: batch {batch} > 65535")
    o = check_out(out, oshape, input.dtype, "conv2d")
    call("pgk_conv2d", input._p, weight._p, packed_weight._p if packed_weight is not None else None,
         bias._p if bias is not None else None, add._p if add is not None else None, o._p, batch, c_in, c_out, h, w, kh, kw,
         s[0], s[1], p[0], p[1], d[0], d[1], int(upsample), 1 if channels_last else 0, 1 if channels_last_out else 0,
         input.dtype.code, None)
    return o


__all__ = ["conv1d", "conv1d_plan", "conv1d_pack_weight", "conv2d", "conv2d_plan", "conv2d_pack_weight"]
