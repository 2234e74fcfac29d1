"""GPU tests of sdpa_causal_fp8 and its per-head quantiser against the restated oracle (tests/fp8_attn_ref.py).

Bars: the quantiser is bit-exact (power-of-two scales, exact multiply).  The attention output must be within
rel_err 1e-2 of the fp8 restatement - the project's bf16 bar: the kernel differs from the restatement only in fp32
summation order, exp2 versus exp and P's rounding to bf16, which the bf16 kernel meets the same bar with.  The
restatement itself is 3e-2 away from the unquantised op on normal data (tests/test_fp8_attn_cpu.py), so a kernel that
quietly ran in bf16 fails."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from oracle import cpu_ref as O
from tests import fp8_attn_ref as R
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu

BAR = 1e-2


def _dev(x):
    from pygpukit_amd.core import from_numpy

    return from_numpy(O.f32_to_bf16_bits(np.ascontiguousarray(x, np.float32)))


def _host(a) -> np.ndarray:
    return O.bf16_bits_to_f32(a.to_numpy())


def _out(shape):
    from pygpukit_amd.core import from_numpy

    return from_numpy(np.full(shape, 0x7FC0, np.uint16))     # bf16 NaN everywhere: every element must be written


# ---- quantiser -------------------------------------------------------------------------------------------------

def _quant_input(h: int, rows: int) -> np.ndarray:
    """Heads scaled by 2^-10 .. 2^10; head 0 carries absmax = 448 * 2^k exactly, RNE ties (17 -> 16, 19 -> 20,
    432 -> 448) and values that reach the largest code only by rounding (446, 434); head 1 is all zero."""
    rng = np.random.default_rng(100 * h + rows)
    x = R.bf16_normal(rng, (h, rows, 128))
    ks = np.round(np.linspace(-10, 10, h)).astype(int)
    x *= (2.0 ** ks)[:, None, None].astype(np.float32)
    x[0, 0, :10] = np.float32([448, 17, 19, 432, 446, -17, -432, 434, -19, 2.0 ** -11]) * np.float32(2.0 ** ks[0])
    x[1] = 0.0
    return x


@functools.lru_cache(maxsize=None)
def _quant_case(h: int, rows: int):
    x = _quant_input(h, rows)
    return x, R.quantize_per_head(x)


@pytest.mark.parametrize("h,rows", [(3, 1), (4, 200), (8, 1030)])
@pytest.mark.parametrize("layout", ["contiguous", "shd"])
def test_quantize_fp8_per_head_is_bit_exact(h, rows, layout):
    from pygpukit_amd import ops

    x, (want_codes, want_sb) = _quant_case(h, rows)
    if layout == "contiguous":
        codes, sb = ops.quantize_fp8_per_head(_dev(x))
    else:
        codes, sb = ops.quantize_fp8_per_head(_dev(x.transpose(1, 0, 2)), strides=(128, h * 128), shape=(h, rows, 128))
    got_codes, got_sb = codes.to_numpy(), sb.to_numpy()
    np.testing.assert_array_equal(got_sb, want_sb)
    assert len(set(want_sb.tolist())) >= 3 and want_sb[1] == 127
    bad = np.argwhere(got_codes != want_codes)
    assert bad.size == 0, [(tuple(i), hex(got_codes[tuple(i)]), hex(want_codes[tuple(i)]), x[tuple(i)]) for i in bad[:8]]
    # the planted values landed where the comment says
    np.testing.assert_array_equal(got_codes[0, 0, :9], [0x7E, 0x58, 0x5A, 0x7E, 0x7E, 0xD8, 0xFE, 0x7E, 0xDA])
    assert not got_codes[1].any()


# ---- attention ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _case(hq, hkv, q_len, kv_len, scale=0.0, seed=0, kind="normal"):
    rng = np.random.default_rng(seed)
    if kind == "integer":
        q, k, v = R.exact_integer_qk(rng, hq, hkv, q_len, kv_len)
    else:
        q, k, v = R.bf16_normal(rng, (hq, q_len, 128)), R.bf16_normal(rng, (hkv, kv_len, 128)), R.bf16_normal(rng, (hkv, kv_len, 128))
        if kind == "zero_q_head":
            q[1] = 0.0
    for a in (q, k, v):
        a.setflags(write=False)
    return q, k, v, R.sdpa_causal_fp8(q, k, v, scale), R.sdpa_causal_unquantised(q, k, v, scale)


def _run(q, k, v, scale=0.0):
    from pygpukit_amd import ops

    out = _out(q.shape)
    assert ops.sdpa_causal_fp8(_dev(q), _dev(k), _dev(v), out, scale) is None
    got = _host(out)
    assert np.isfinite(got).all()
    return got


SHAPES = [
    (4, 4, 200, 200),      # partial query tile and partial KV tile
    (4, 2, 200, 200),      # GQA
    (2, 2, 1, 70),
    (8, 8, 129, 333),      # prefix offset, second query tile one row wide
    (2, 1, 512, 512),      # 2 KV runs per query tile (the launcher's heuristic on 256 CUs)
    (2, 1, 600, 1100),     # 4 KV runs
]


@pytest.mark.parametrize("hq,hkv,q_len,kv_len", SHAPES)
def test_sdpa_causal_fp8_matches_the_restatement(hq, hkv, q_len, kv_len):
    q, k, v, want, _ = _case(hq, hkv, q_len, kv_len)
    err = rel_err(_run(q, k, v), want)
    print(f"sdpa_causal_fp8 {(hq, hkv, q_len, kv_len)}: rel_err to the fp8 restatement {err:.3e}")
    assert err <= BAR


def test_explicit_scale():
    q, k, v, want, _ = _case(4, 2, 130, 200, scale=0.2, seed=3)
    err = rel_err(_run(q, k, v, 0.2), want)
    print(f"explicit scale 0.2: rel_err {err:.3e}")
    assert err <= BAR


def test_strided_entry_with_q_and_out_in_shd_layout():
    from pygpukit_amd import ops

    hq, hkv, q_len, kv_len = 4, 2, 200, 200
    q, k, v, want, _ = _case(hq, hkv, q_len, kv_len)
    out = _out((q_len, hq, 128))
    ops.sdpa_causal_fp8_strided(_dev(q.transpose(1, 0, 2)), _dev(k), _dev(v), out, hq, hkv, q_len, kv_len, 128,
                                (128, hq * 128), (kv_len * 128, 128), (128, hq * 128))
    err = rel_err(_host(out).transpose(1, 0, 2), want)
    print(f"strided entry: rel_err {err:.3e}")
    assert err <= BAR


def test_all_zero_q_head_gives_the_running_mean_of_v():
    q, k, v, want, _ = _case(4, 4, 200, 200, seed=5, kind="zero_q_head")
    got = _run(q, k, v)
    assert rel_err(got, want) <= BAR
    mean = np.cumsum(v[1].astype(np.float64), axis=0) / np.arange(1, 201)[:, None]
    assert rel_err(got[1], mean) <= BAR


def test_the_fp8_path_is_really_taken():
    q, k, v, want, unq = _case(4, 4, 200, 200)
    got = _run(q, k, v)
    to_fp8, to_unq = rel_err(got, want), rel_err(got, unq)
    print(f"rel_err to the fp8 restatement {to_fp8:.3e}, to the unquantised oracle {to_unq:.3e}")
    assert to_fp8 <= BAR
    assert to_unq >= 2e-2


@pytest.mark.parametrize("hq,hkv,q_len,kv_len", [(2, 1, 150, 150), (2, 2, 96, 160)])
def test_operand_layout_on_exact_integer_data(hq, hkv, q_len, kv_len):
    """Integer Q, K survive the quantisation exactly, so the result must match the UNQUANTISED oracle: a wrong A / B lane
    map or a swapped k order of the fp8 MFMA pairs the wrong d and fails outright."""
    q, k, v, _, unq = _case(hq, hkv, q_len, kv_len, scale=1.0 / 256, seed=11, kind="integer")
    err = rel_err(_run(q, k, v, 1.0 / 256), unq)
    print(f"exact-integer {(hq, hkv, q_len, kv_len)}: rel_err to the unquantised oracle {err:.3e}")
    assert err <= BAR


# ---- public surface ----------------------------------------------------------------------------------------------

def test_public_surface():
    import pygpukit_amd as pk
    from pygpukit_amd.core import from_numpy

    assert pk.fa3_fp8_available() is True
    assert pk.get_sm_version() == 950
    bf = lambda *s: from_numpy(np.zeros(s, np.uint16))     # noqa: E731
    with pytest.raises(ValueError):
        pk.sdpa_causal_fp8(bf(2, 8, 64), bf(2, 8, 64), bf(2, 8, 64), bf(2, 8, 64))
    h = lambda *s: from_numpy(np.zeros(s, np.float16))     # noqa: E731
    with pytest.raises(ValueError):
        pk.sdpa_causal_fp8(h(2, 8, 128), h(2, 8, 128), h(2, 8, 128), h(2, 8, 128))
    with pytest.raises(ValueError):
        pk.sdpa_causal_fp8(bf(3, 8, 128), bf(2, 8, 128), bf(2, 8, 128), bf(3, 8, 128))
    with pytest.raises(ValueError):
        pk.sdpa_causal_fp8(bf(2, 8, 128), bf(2, 8, 128), bf(2, 8, 128), bf(2, 9, 128))
    with pytest.raises(ValueError, match="kv_len >= q_len"):
        pk.sdpa_causal_fp8(bf(2, 9, 128), bf(2, 8, 128), bf(2, 8, 128), bf(2, 9, 128))
    with pytest.raises(ValueError):
        pk.ops.sdpa_causal_fp8_strided(bf(2, 8, 128), bf(2, 8, 128), bf(2, 8, 128), bf(2, 8, 128), 3, 2, 8, 8, 128, (1024, 128), (1024, 128), (1024, 128))
    # the native entry refuses the same on its own, with a message
    from pygpukit_amd import _hip

    x = bf(2, 8, 64)
    with pytest.raises(RuntimeError, match="head_dim must be 128"):
        _hip.call("pgk_sdpa_causal_fp8", x._p, x._p, x._p, x._p, 2, 2, 8, 8, 64, 0.0, 512, 64, 512, 64, 512, 64, x.dtype.code, None)
