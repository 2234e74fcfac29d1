"""[build-defined] patchify / unpatchify: the two reshapes of the reference's models/dit/embeddings.py (patch_embed, unpatchify),
which it runs on the host, as device moves (csrc/ops_diffusion.hip)."""

from __future__ import annotations

from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.ops._common import call, check_out


def _check(op: str, H: int, W: int, p: int) -> None:
    if p < 1:
        raise ValueError(f"{op}: patch_size must be >= 1, got {p}")
    if H % p or W % p:
        raise ValueError(f"{op}: H={H} and W={W} must be multiples of the patch size {p}")


def patchify(x: GPUArray, patch_size: int, *, out: GPUArray | None = None) -> GPUArray:
    """[B, C, H, W] -> [B * hp * wp, C * p * p]: rows in row-major (h, w) patch order, columns (c, ph, pw)."""
    if x.ndim != 4 or x.itemsize not in (2, 4):
        raise ValueError(f"patchify expects a 4D [B, C, H, W] array of 2- or 4-byte elements, got {x.shape} {x.dtype.name}")
    B, C, H, W = x.shape
    p = int(patch_size)
    _check("patchify", H, W, p)
    o = check_out(out, (B * (H // p) * (W // p), C * p * p), x.dtype, "patchify")
    call("pgk_patchify", x._p, o._p, B, C, H, W, p, x.dtype.code, None)
    return o


def unpatchify(x: GPUArray, batch: int, out_channels: int, H: int, W: int, patch_size: int, *, out: GPUArray | None = None) -> GPUArray:
    """[B * hp * wp, p * p * Co] with columns (ph, pw, c) -> [B, Co, H, W]."""
    p = int(patch_size)
    _check("unpatchify", H, W, p)
    want = (batch * (H // p) * (W // p), p * p * out_channels)
    if x.itemsize not in (2, 4) or x.size != want[0] * want[1] or x.shape[-1] != want[1]:
        raise ValueError(f"unpatchify expects {want} of 2- or 4-byte elements, got {x.shape} {x.dtype.name}")
    o = check_out(out, (batch, out_channels, H, W), x.dtype, "unpatchify")
    call("pgk_unpatchify", x._p, o._p, batch, out_channels, H, W, p, x.dtype.code, None)
    return o


__all__ = ["patchify", "unpatchify"]
