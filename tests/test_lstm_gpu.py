"""lstm_forward / lstm_bidirectional on the GPU against the float64 oracle (tests/lstm_ref.py, itself checked against
torch.nn.LSTM's recorded results in test_lstm_cpu.py), on both recurrence paths (PGK_LSTM_RESIDENT unset and =0).

Bars.  float32: max|gpu - ref64| <= BAR32 = K * max|ref32 - ref64| over output, h_n and c_n together, where ref32 is the
NumPy float32 evaluation of the same inputs (never the code under test), and BAR32 <= 1e-4 is a condition on every case.
bfloat16 / float16: the oracle is ref64 on the 16-bit-rounded inputs and |gpu - ref| <= 2^-8 |ref| + BAR32 (bf16) or
2^-11 |ref| + BAR32 (f16): half an ulp of the returned value plus the fp32 arithmetic, because the state is never rounded.
test_lstm_cpu.py shows that every planted error moves the output by >= 0.1, a thousand times the cap.

K = 8, measured on an MI355X over every case below, both paths: the worst (|gpu - ref64| - rounding term) / max|ref32 - ref64|
was 2.52 in float32 ((1,16,512,256) bidirectional c_n: 8.6e-7 against 3.4e-7; per shape 1.0, 2.1, 2.1, 1.7, 2.0, 2.5, 1.2 in
the order of the list; resident and stepped alike), 0.09 in bfloat16 and 0.16 in float16.  K is the smallest power of two that
is at least twice the worst ratio (2 x 2.52 = 5.0 -> 8); the largest BAR32 of any case is then 8 x 6.2e-7 = 5.0e-6.

The chained call (S split in two, (h_n, c_n) handed on as (h0, c0)) is checked in float32 only, with the same bar: there the
hand-over loses nothing.  In the 16-bit dtypes the returned state is rounded to 16 bits (|c| up to ~3 -> up to 2^-8 * 3 of
error injected into the second half), which is the contract, not an error of the kernels, and no derivable bar covers it."""

from __future__ import annotations

import functools

import numpy as np
import pytest

import pygpukit_amd as pk
from pygpukit_amd.core.dtypes import bfloat16, float16, float32
from pygpukit_amd.ops.nn import lstm_bidirectional, lstm_forward
from pygpukit_amd.ops.nn.recurrent import lstm_plan
from tests import lstm_ref as R

pytestmark = pytest.mark.gpu

K = 8
CAP = 1e-4
REL = {"float32": 0.0, "bfloat16": 2.0 ** -8, "float16": 2.0 ** -11}
DTYPES = {"float32": float32, "bfloat16": bfloat16, "float16": float16}
PATHS = ("default", "stepped")                      # PGK_LSTM_RESIDENT unset / "0"
CASES = [(s, dt) for s in R.GPU_SHAPES for dt in DTYPES if dt == "float32" or (s[2] % 8 == 0 and s[3] % 8 == 0)]
UNI_KEYS = ("x", "W_ih", "W_hh", "b_ih", "b_hh", "h0", "c0")


# ---- host <-> device in the three dtypes ------------------------------------------------------------------------------
def _bits(a: np.ndarray, dt: str) -> np.ndarray:
    """float64 -> the storage words the device gets (bf16: RNE, as uint16)."""
    if dt == "float32":
        return a.astype(np.float32)
    if dt == "float16":
        return a.astype(np.float16)
    u = np.ascontiguousarray(a.astype(np.float32)).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _value(bits: np.ndarray, dt: str) -> np.ndarray:
    if dt == "bfloat16":
        return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return bits.astype(np.float64)


@functools.lru_cache(maxsize=None)
def _case(shape, dt: str, bidir: bool):
    """(storage words, their float64 values) of one case's inputs; the oracle sees exactly what the device gets."""
    d = R.make_bidir_case(*shape, seed=R.case_seed(shape) + 1) if bidir else R.make_case(*shape, seed=R.case_seed(shape))
    bits = {k: _bits(v, dt) for k, v in d.items()}
    return bits, {k: _value(v, dt) for k, v in bits.items()}


@functools.lru_cache(maxsize=None)
def _oracle(shape, dt: str, reverse: bool, state: bool):
    """(ref64 triple, BAR32) of a unidirectional configuration, computed once and shared."""
    _, v = _case(shape, dt, False)
    args = [v[k] for k in UNI_KEYS[:5]] + ([v["h0"], v["c0"]] if state else [None, None])
    ref = R.lstm_forward(*args, reverse=reverse)
    r32 = R.lstm_forward(*args, reverse=reverse, dtype=np.float32)
    return ref, K * _maxdev(r32, ref), _maxdev(r32, ref)


@functools.lru_cache(maxsize=None)
def _oracle_bidir(shape, dt: str):
    """per direction: (ref64 triple, BAR32)."""
    _, v = _case(shape, dt, True)
    res = []
    for sfx, rev in (("_fwd", False), ("_bwd", True)):
        args = [v["x"]] + [v[k + sfx] for k in R.WEIGHTS]
        ref = R.lstm_forward(*args, reverse=rev)
        r32 = R.lstm_forward(*args, reverse=rev, dtype=np.float32)
        res.append((ref, K * _maxdev(r32, ref), _maxdev(r32, ref)))
    return res


def _maxdev(a, b) -> float:
    return max(float(np.max(np.abs(np.asarray(x, np.float64) - np.asarray(y, np.float64)))) for x, y in zip(a, b))


def _set_path(monkeypatch, path: str) -> None:
    if path == "stepped":
        monkeypatch.setenv("PGK_LSTM_RESIDENT", "0")
    else:
        monkeypatch.delenv("PGK_LSTM_RESIDENT", raising=False)


def _check(got_bits, ref, bar32: float, dev32: float, dt: str, what: str) -> None:
    """got_bits: (out, h_n, c_n) storage words from the device."""
    assert 0 < bar32 <= CAP, (what, bar32)
    for name, g, r in zip(("output", "h_n", "c_n"), got_bits, ref):
        err = np.abs(_value(g, dt) - r)
        allowed = REL[dt] * np.abs(r) + bar32
        worst = float(np.max(err - REL[dt] * np.abs(r)))
        print(f"LSTM-RATIO {what} {name}: max err {float(err.max()):.3e} excess-over-rounding/dev32 {worst / dev32:.2f} (dev32 {dev32:.2e})")
        assert np.all(err <= allowed), (what, name, float(np.max(err - allowed)), bar32)


def _np(arrs):
    return tuple(a.to_numpy() for a in arrs)


# ---- every shape, dtype and path ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("shape,dt", CASES, ids=[f"{s}-{d}" for s, d in CASES])
def test_lstm_forward(shape, dt, path, monkeypatch):
    _set_path(monkeypatch, path)
    B, S, I, H = shape
    if path == "stepped":
        assert lstm_plan(B, H, dt) == "stepped"
    bits, _ = _case(shape, dt, False)
    dev = {k: pk.from_numpy(bits[k]) for k in UNI_KEYS}
    assert all(a.dtype == DTYPES[dt] for a in dev.values())
    w = [dev[k] for k in UNI_KEYS[:5]]
    for reverse in (False, True):
        for state in (True, False):
            h0c0 = (dev["h0"], dev["c0"]) if state else (None, None)
            res = lstm_forward(*w, *h0c0, reverse=reverse)
            assert [a.shape for a in res] == [(B, S, H), (B, H), (B, H)] and all(a.dtype == DTYPES[dt] for a in res)
            got = _np(res)
            ref, bar32, dev32 = _oracle(shape, dt, reverse, state)
            _check(got, ref, bar32, dev32, dt, f"{shape} {dt} {path} rev={reverse} state={state}")
            # h_n is the last-processed output row, bit for bit
            assert np.array_equal(got[1], got[0][:, 0 if reverse else -1])
            # the same call again: the same bytes
            again = _np(lstm_forward(*w, *h0c0, reverse=reverse))
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    for k in UNI_KEYS:                                   # inputs untouched
        assert dev[k].to_numpy().tobytes() == bits[k].tobytes(), k


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("shape,dt", CASES, ids=[f"{s}-{d}" for s, d in CASES])
def test_lstm_bidirectional(shape, dt, path, monkeypatch):
    _set_path(monkeypatch, path)
    B, S, I, H = shape
    bits, _ = _case(shape, dt, True)
    dev = {k: pk.from_numpy(v) for k, v in bits.items()}
    res = lstm_bidirectional(*R.bidir_args(dev))
    assert [a.shape for a in res] == [(B, S, 2 * H), (2, B, H), (2, B, H)] and all(a.dtype == DTYPES[dt] for a in res)
    out, hn, cn = _np(res)
    for d, (ref, bar32, dev32) in enumerate(_oracle_bidir(shape, dt)):
        o = out[..., d * H:(d + 1) * H]
        _check((o, hn[d], cn[d]), ref, bar32, dev32, dt, f"{shape} {dt} {path} bidir dir={d}")
        assert np.array_equal(hn[d], o[:, 0 if d else -1])
    again = _np(lstm_bidirectional(*R.bidir_args(dev)))
    assert all(a.tobytes() == b.tobytes() for a, b in zip((out, hn, cn), again))
    for k, v in bits.items():
        assert dev[k].to_numpy().tobytes() == v.tobytes(), k


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("reverse", (False, True))
@pytest.mark.parametrize("shape", [s for s in R.GPU_SHAPES if s[1] >= 2], ids=str)
def test_chained_halves_match_the_whole_call(shape, reverse, path, monkeypatch):
    _set_path(monkeypatch, path)
    B, S, I, H = shape
    bits, _ = _case(shape, "float32", False)
    dev = {k: pk.from_numpy(bits[k]) for k in UNI_KEYS}
    w = [dev[k] for k in UNI_KEYS[1:5]]
    cut = S // 2
    halves = [pk.from_numpy(np.ascontiguousarray(bits["x"][:, :cut])), pk.from_numpy(np.ascontiguousarray(bits["x"][:, cut:]))]
    order = (1, 0) if reverse else (0, 1)
    o1, h1, c1 = lstm_forward(halves[order[0]], *w, dev["h0"], dev["c0"], reverse=reverse)
    o2, h2, c2 = lstm_forward(halves[order[1]], *w, h1, c1, reverse=reverse)
    parts = {order[0]: o1.to_numpy(), order[1]: o2.to_numpy()}
    got = (np.concatenate([parts[0], parts[1]], axis=1), h2.to_numpy(), c2.to_numpy())
    ref, bar32, dev32 = _oracle(shape, "float32", reverse, True)
    _check(got, ref, bar32, dev32, "float32", f"{shape} chained {path} rev={reverse}")


# ---- both paths really ran ---------------------------------------------------------------------------------------------
def test_both_paths_are_covered_in_every_dtype(monkeypatch):
    for dt in DTYPES:
        shapes = [s for s, d in CASES if d == dt]
        monkeypatch.delenv("PGK_LSTM_RESIDENT", raising=False)
        assert {lstm_plan(s[0], s[3], dt) for s in shapes} == {"resident", "stepped"}, dt
        monkeypatch.setenv("PGK_LSTM_RESIDENT", "0")
        assert {lstm_plan(s[0], s[3], dt) for s in shapes} == {"stepped"}, dt
    monkeypatch.delenv("PGK_LSTM_RESIDENT", raising=False)
    assert lstm_plan(5, 128, "float32") == "resident"          # the largest H claimed resident, in the list above
    assert lstm_plan(1, 256, "float32") == "stepped"           # the Kokoro encoder shape


def test_golden_case_on_the_gpu():
    """torch.nn.LSTM's own recorded numbers, not only the restatement: float32 inputs are the float64 fixture rounded."""
    from tests.conftest import load_golden

    g = load_golden("g9_lstm.npz")
    args64 = [g["u_" + k].astype(np.float32).astype(np.float64) for k in UNI_KEYS]
    for reverse, sfx in ((False, ""), (True, "_rev")):
        ref = R.lstm_forward(*args64, reverse=reverse)
        dev32 = _maxdev(R.lstm_forward(*args64, reverse=reverse, dtype=np.float32), ref)
        # rounding the inputs to float32 moves torch's float64 result by a few 1e-7: the recorded numbers bound the oracle
        assert _maxdev(ref, (g["u_out" + sfx], g["u_hn" + sfx], g["u_cn" + sfx])) < 1e-5
        got = _np(lstm_forward(*[pk.from_numpy(g["u_" + k].astype(np.float32)) for k in UNI_KEYS], reverse=reverse))
        _check(got, ref, K * dev32, dev32, "float32", f"golden rev={reverse}")
