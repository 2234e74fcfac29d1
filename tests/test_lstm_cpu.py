"""LSTM ops without a GPU: the NumPy oracle (tests/lstm_ref.py) against torch.nn.LSTM's recorded float64 results
(tests/golden/g9_lstm.npz), the proof that the GPU test's bars separate a right LSTM from a wrong one, the exported
surface, the host-only plan query and the argument checks (which run before anything touches a device)."""

from __future__ import annotations

import numpy as np
import pytest

from pygpukit_amd import _hip
from pygpukit_amd.core.array import GPUArray
from pygpukit_amd.core.dtypes import bfloat16, float16, float32, int32
from pygpukit_amd.ops.nn import lstm_bidirectional, lstm_forward
from pygpukit_amd.ops.nn.recurrent import lstm_plan
from tests import lstm_ref as R
from tests.conftest import load_golden

g9 = load_golden("g9_lstm.npz")
CAP = 1e-4                       # the most BAR32 may ever be (tests/test_lstm_gpu.py)


def _uni(prefix="u_"):
    return [g9[prefix + k] for k in ("x", "W_ih", "W_hh", "b_ih", "b_hh", "h0", "c0")]


def _dev(got, want):
    return max(float(np.max(np.abs(np.asarray(g, np.float64) - w))) for g, w in zip(got, want))


# ---- oracle against the fixture -------------------------------------------------------------------------------------
def test_ref64_matches_torch_unidirectional():
    assert g9["u_x"].shape == (2, 5, 24) and g9["u_W_hh"].shape == (80, 20)
    assert _dev(R.lstm_forward(*_uni()), (g9["u_out"], g9["u_hn"], g9["u_cn"])) <= 1e-12
    assert _dev(R.lstm_forward(*_uni(), reverse=True), (g9["u_out_rev"], g9["u_hn_rev"], g9["u_cn_rev"])) <= 1e-12


def test_ref64_matches_torch_bidirectional():
    d = {k[2:]: g9[k] for k in g9.files if k.startswith("b_")}
    assert d["x"].shape == (2, 6, 16) and d["out"].shape == (2, 6, 16)
    assert _dev(R.lstm_bidirectional(*R.bidir_args(d)), (d["out"], d["hn"], d["cn"])) <= 1e-12


def test_ref32_mode_is_float32_and_close():
    # 16 x the largest float32-vs-float64 deviation of this restatement on the test distribution (5.1e-7): only to show
    # that the mode really computes in float32 and computes the same thing
    got = R.lstm_forward(*_uni(), dtype=np.float32)
    assert all(a.dtype == np.float32 for a in got)
    dev = _dev(got, (g9["u_out"], g9["u_hn"], g9["u_cn"]))
    assert 1e-9 < dev <= 16 * 5.1e-7, dev
    d = {k[2:]: g9[k] for k in g9.files if k.startswith("b_")}
    dev = _dev(R.lstm_bidirectional(*R.bidir_args(d), dtype=np.float32), (d["out"], d["hn"], d["cn"]))
    assert 1e-9 < dev <= 16 * 5.1e-7, dev


def test_reverse_convention():
    out, hn, _ = R.lstm_forward(*_uni(), reverse=True)
    assert np.array_equal(hn, out[:, 0])
    out, hn, _ = R.lstm_forward(*_uni())
    assert np.array_equal(hn, out[:, -1])


# ---- the bars separate right from wrong -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [s for s in R.GPU_SHAPES if s[3] >= 20], ids=str)
def test_every_planted_error_moves_the_output_far_beyond_the_bars(shape):
    d = R.make_case(*shape, seed=R.case_seed(shape))
    args = [d[k] for k in ("x", "W_ih", "W_hh", "b_ih", "b_hh", "h0", "c0")]
    right = {rev: R.lstm_forward(*args, reverse=rev)[0] for rev in (False, True)}
    for m in R.MUTATIONS:
        rev = m == "no_reverse"
        moved = float(np.max(np.abs(R.lstm_forward(*args, reverse=rev, mutate=m)[0] - right[rev])))
        # >= 0.1: 1000 x the 1e-4 cap on BAR32 and 10 x the bf16 bar at |c| = 2.5 (2^-8 * 2.5 + 1e-4 = 0.0099)
        assert moved >= 0.1, (m, moved)
        assert moved > 10 * (2.0 ** -8 * 2.5 + CAP)


def test_unknown_mutation_is_rejected():
    with pytest.raises(ValueError):
        R.lstm_forward(*_uni(), mutate="swap_xy")


# ---- exported surface -------------------------------------------------------------------------------------------------
def test_library_exports_the_entries():
    lib = _hip.load()
    for name in ("pgk_lstm", "pgk_lstm_plan"):
        assert name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name)


def test_names_importable_where_the_reference_has_them():
    import pygpukit_amd
    from pygpukit_amd import ops
    from pygpukit_amd.ops import basic, nn

    for mod in (nn, ops, basic, pygpukit_amd):
        assert mod.lstm_forward is lstm_forward and mod.lstm_bidirectional is lstm_bidirectional
    assert "lstm_forward" in nn.__all__ and "lstm_bidirectional" in nn.__all__
    assert "lstm_forward" in basic.__all__ and "lstm_bidirectional" in ops.__all__


# ---- plan query (host only) -------------------------------------------------------------------------------------------
def test_plan_default(monkeypatch):
    monkeypatch.delenv("PGK_LSTM_RESIDENT", raising=False)
    assert lstm_plan(1, 64, "float32") == "resident"
    assert lstm_plan(1, 256, "float32") == "stepped"
    for dt in (float32, bfloat16, float16):
        assert lstm_plan(5, 128, dt) == "resident"
        assert lstm_plan(2, 136, dt) == "stepped"
        assert lstm_plan(1, 1, float32) == "resident"


def test_plan_switch_forces_stepped(monkeypatch):
    monkeypatch.setenv("PGK_LSTM_RESIDENT", "0")
    for dt in (float32, bfloat16, float16):
        for h in (1, 8, 20, 64, 128, 136, 256, 1024):
            for b in (1, 4, 11):
                assert lstm_plan(b, h, dt) == "stepped"
    monkeypatch.setenv("PGK_LSTM_RESIDENT", "1")
    assert lstm_plan(1, 64, float32) == "resident" and lstm_plan(1, 256, float32) == "stepped"


# ---- argument checks: ValueError naming the argument, before any device call --------------------------------------------
def _fake(shape, dtype=float32):
    return GPUArray(shape, dtype, device_ptr=0x1000, owns_memory=False)     # never dereferenced: the checks come first


def _args(B=2, S=3, I=16, H=8, dt=float32, **over):
    a = dict(x=_fake((B, S, I), dt), W_ih=_fake((4 * H, I), dt), W_hh=_fake((4 * H, H), dt), b_ih=_fake((4 * H,), dt),
             b_hh=_fake((4 * H,), dt), h0=_fake((B, H), dt), c0=_fake((B, H), dt))
    a.update(over)
    return a


BAD = [
    ("x", dict(x=_fake((3, 16)))),                                    # not 3-D
    ("x", dict(x=_fake((2, 0, 16)))),                                 # empty dimension
    ("x", dict(x=_fake((0, 3, 16)), h0=None, c0=None)),
    ("W_ih", dict(W_ih=_fake((24, 16)))),                             # W_ih.shape[0] != 4 * W_hh.shape[1]
    ("W_ih", dict(W_ih=_fake((32, 24)))),                             # input size does not fit x
    ("W_ih", dict(W_ih=_fake((32,)))),
    ("W_hh", dict(W_hh=_fake((24, 8)))),
    ("W_hh", dict(W_hh=_fake((32, 0)))),
    ("b_ih", dict(b_ih=_fake((8,)))),
    ("b_hh", dict(b_hh=_fake((32, 1)))),
    ("h0", dict(h0=_fake((3, 8)))),
    ("c0", dict(c0=_fake((2, 4)))),
    ("W_hh", dict(W_hh=_fake((32, 8), bfloat16))),                    # mixed dtypes
    ("c0", dict(c0=_fake((2, 8), float16))),
    ("x", dict(x=_fake((2, 3, 16), int32))),                          # non-float
]


@pytest.mark.parametrize("arg,over", BAD, ids=[f"{i}-{a}" for i, (a, _) in enumerate(BAD)])
def test_forward_rejects(arg, over):
    with pytest.raises(ValueError, match=arg):
        lstm_forward(**_args(**over))


@pytest.mark.parametrize("dt", [bfloat16, float16], ids=str)
def test_16bit_sizes_must_be_multiples_of_8(dt):
    with pytest.raises(ValueError, match="x"):
        lstm_forward(**_args(I=12, dt=dt))
    with pytest.raises(ValueError, match="W_hh"):
        lstm_forward(**_args(H=20, dt=dt))


def test_bidirectional_rejects():
    a = _args()
    base = dict(x=a["x"], **{f"{k}_{d}": a[k] for k in R.WEIGHTS for d in ("fwd", "bwd")})
    for key, bad in (("W_ih_bwd", _fake((24, 16))), ("b_hh_fwd", _fake((31,))), ("W_hh_bwd", _fake((64, 16))),
                     ("b_ih_bwd", _fake((32,), float16)), ("x", _fake((2, 3)))):
        with pytest.raises(ValueError, match=key.split("_bwd")[0] if key == "W_hh_bwd" else key):
            lstm_bidirectional(**{**base, key: bad})
