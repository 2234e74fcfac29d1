"""LSTM forward over a whole sequence (reference: src/pygpukit/ops/nn/recurrent.py, native/ops/nn/recurrent/lstm.inl).

    g   = W_ih . x_t + b_ih + b_hh + W_hh . h_{t-1}          gate order i, f, g, o (PyTorch)
    c_t = sigmoid(f) * c_{t-1} + sigmoid(i) * tanh(g_g)       h_t = sigmoid(o) * tanh(c_t)

One C entry (pgk_lstm, csrc/ops_lstm.hip) serves one or two directions: the gate projection of every timestep and both
directions is one launch, the recurrence is one more launch when W_hh fits one workgroup ("resident", H <= 128) and one
launch per timestep for both directions and all batch rows otherwise ("stepped").  float32 is the reference's contract;
float16 / bfloat16 are [build-defined] (I % 8 == 0, H % 8 == 0).  In every dtype gates, h and c are fp32 for the whole
sequence and only the returned tensors are rounded.  Nothing synchronises the host.  Contract: INTEGRATION.md."""

from __future__ import annotations

import ctypes as C

from pygpukit_amd import _hip
from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import DataType, as_dtype, float32
from pygpukit_amd.ops._common import call, validate_float


def lstm_plan(batch: int, hidden: int, dtype: "str | DataType" = float32) -> str:
    """Which recurrence a call of this size takes under the current environment (PGK_LSTM_RESIDENT=0 forces "stepped"):
    host logic only, needs no device."""
    return "resident" if _hip.load().pgk_lstm_plan(int(batch), int(hidden), as_dtype(dtype).code) else "stepped"


def _check_dir(x: GPUArray, W_ih: GPUArray, W_hh: GPUArray, b_ih: GPUArray, b_hh: GPUArray, h0, c0, name: str, sfx: str = "") -> int:
    """Validate one direction's operands against x [B, S, I]; returns H."""
    batch, _, isz = x.shape
    for arg, a in (("W_ih", W_ih), ("W_hh", W_hh)):
        if a.ndim != 2:
            raise ValueError(f"{name}: {arg}{sfx} must be 2D, got shape {a.shape}")
    hidden = W_hh.shape[1]
    if hidden < 1:
        raise ValueError(f"{name}: W_hh{sfx} has an empty dimension, shape {W_hh.shape}")
    if W_ih.shape[0] != 4 * hidden:
        raise ValueError(f"{name}: W_ih{sfx} must have 4 * hidden_size = {4 * hidden} rows (W_hh{sfx} is {W_hh.shape}), got {W_ih.shape}")
    if W_ih.shape[1] != isz:
        raise ValueError(f"{name}: W_ih{sfx} must be [{4 * hidden}, {isz}] for x {x.shape}, got {W_ih.shape}")
    if W_hh.shape[0] != 4 * hidden:
        raise ValueError(f"{name}: W_hh{sfx} must be [{4 * hidden}, {hidden}], got {W_hh.shape}")
    for arg, a in (("b_ih", b_ih), ("b_hh", b_hh)):
        if a.shape != (4 * hidden,):
            raise ValueError(f"{name}: {arg}{sfx} must be [{4 * hidden}], got {a.shape}")
    for arg, a in (("h0", h0), ("c0", c0)):
        if a is not None and a.shape != (batch, hidden):
            raise ValueError(f"{name}: {arg} must be [{batch}, {hidden}], got {a.shape}")
    for arg, a in (("W_ih", W_ih), ("W_hh", W_hh), ("b_ih", b_ih), ("b_hh", b_hh), ("h0", h0), ("c0", c0)):
        if a is not None and a.dtype != x.dtype:
            raise ValueError(f"{name}: {arg}{sfx if arg[0] in 'Wb' else ''} has dtype {a.dtype}, x has {x.dtype} (all tensors share one dtype)")
    if x.dtype != float32:
        if isz % 8:
            raise ValueError(f"{name}: x input_size must be a multiple of 8 for {x.dtype}, got {isz}")
        if hidden % 8:
            raise ValueError(f"{name}: W_hh{sfx} hidden_size must be a multiple of 8 for {x.dtype}, got {hidden}")
    return hidden


def _check_x(x: GPUArray, name: str) -> None:
    if x.ndim != 3:
        raise ValueError(f"{name}: x must be 3D [batch, seq_len, input_size], got {x.ndim}D")
    validate_float(x, f"{name}: x")
    if 0 in x.shape:
        raise ValueError(f"{name}: x has an empty dimension, shape {x.shape}")


def _dir(W_ih, W_hh, b_ih, b_hh, h0=None, c0=None) -> _hip.LstmDir:
    return _hip.LstmDir(W_ih._ptr, W_hh._ptr, b_ih._ptr, b_hh._ptr, h0._ptr if h0 is not None else None,
                        c0._ptr if c0 is not None else None)


def _run(x: GPUArray, fwd: _hip.LstmDir, bwd, hidden: int, reverse: bool):
    batch, seq, isz = x.shape
    ndir = 2 if bwd is not None else 1
    state_shape = (batch, hidden) if ndir == 1 else (2, batch, hidden)
    out = GPUArray((batch, seq, ndir * hidden), x.dtype)
    h_n, c_n = GPUArray(state_shape, x.dtype), GPUArray(state_shape, x.dtype)
    gates = GPUArray((ndir * batch * seq * 4 * hidden,), float32)         # W_ih . x + biases, fp32, every timestep
    state = GPUArray((3 * ndir * batch * hidden,), float32)               # stepped path: h ping-pong and c
    call("pgk_lstm", x._p, C.byref(fwd), C.byref(bwd) if bwd is not None else None, out._p, h_n._p, c_n._p, gates._p, state._p,
         batch, seq, isz, hidden, 1 if reverse else 0, x.dtype.code, None)
    return out, h_n, c_n


def lstm_forward(x: GPUArray, W_ih: GPUArray, W_hh: GPUArray, b_ih: GPUArray, b_hh: GPUArray, h0: GPUArray | None = None,
                 c0: GPUArray | None = None, reverse: bool = False) -> tuple[GPUArray, GPUArray, GPUArray]:
    """x [B, S, I], W_ih [4H, I], W_hh [4H, H], b_ih / b_hh [4H], h0 / c0 [B, H] or None for zeros ->
    (output [B, S, H], h_n [B, H], c_n [B, H]).  reverse=True walks t = S-1 .. 0 and writes output[:, t] at the position
    processed, so h_n is output[:, 0] when reversed and output[:, -1] otherwise."""
    _check_x(x, "lstm_forward")
    hidden = _check_dir(x, W_ih, W_hh, b_ih, b_hh, h0, c0, "lstm_forward")
    return _run(x, _dir(W_ih, W_hh, b_ih, b_hh, h0, c0), None, hidden, bool(reverse))


def lstm_bidirectional(x: GPUArray, W_ih_fwd: GPUArray, W_hh_fwd: GPUArray, b_ih_fwd: GPUArray, b_hh_fwd: GPUArray,
                       W_ih_bwd: GPUArray, W_hh_bwd: GPUArray, b_ih_bwd: GPUArray,
                       b_hh_bwd: GPUArray) -> tuple[GPUArray, GPUArray, GPUArray]:
    """Both directions from zero state in the same launches -> (output [B, S, 2H] with forward in [..., :H] and backward in
    [..., H:], h_n [2, B, H], c_n [2, B, H])."""
    _check_x(x, "lstm_bidirectional")
    hidden = _check_dir(x, W_ih_fwd, W_hh_fwd, b_ih_fwd, b_hh_fwd, None, None, "lstm_bidirectional", "_fwd")
    hidden_b = _check_dir(x, W_ih_bwd, W_hh_bwd, b_ih_bwd, b_hh_bwd, None, None, "lstm_bidirectional", "_bwd")
    if hidden_b != hidden:
        raise ValueError(f"lstm_bidirectional: W_hh_bwd hidden_size {hidden_b} differs from W_hh_fwd's {hidden}")
    return _run(x, _dir(W_ih_fwd, W_hh_fwd, b_ih_fwd, b_hh_fwd), _dir(W_ih_bwd, W_hh_bwd, b_ih_bwd, b_hh_bwd), hidden, False)


__all__ = ["lstm_forward", "lstm_bidirectional", "lstm_plan"]
