"""GPU tests of sdpa_relbias: attention with a clamped relative-position bias table, on the flash kernel's FlashRelBias policy
(bfloat16 / float16, head_dim 64 / 128) and on the one-wave-per-row fp32 kernel (float32, other head dims, unaligned buffers).

Exact key selection.  A table that is -1e4 everywhere except 0 at one delta d0 makes p exactly 1 for key i + d0 and exactly 0
(exp2 of less than -14000) for every other key of row i, so the row must equal V[i + d0] bit for bit: a wrong table index, tile
class or saturated value anywhere on the row's walk selects another key or none.  The clamped edge is selected the same way with
Q = 0: the row is the exact mean of keys 0..i - R, compared at one 16-bit ulp.

Numerical parity.  rel_err <= 1e-2 against the float64 restatement (tests/t5_ref.py) on 16-bit-rounded inputs, the bar and metric
of tests/test_posenc_gpu.py; the float32 rows kernel against t5_ref.f32_bar (derivation there).  Scale 1.0 is T5's: its q / k come
out of projections that fold 1/sqrt(d) into the weights, so the cases at scale 1.0 draw Q and K at D^-1/4 and the scores are of
order one at either scale.

Shapes: a single ragged tile (31 / 31), near and straddling tiles (129 / 200), far-left and far-right uniform tiles (300 / 300 at
radius 40), kv_len < q_len (160 / 131), q_len = 1, and more than one KV run (2 heads, 130 / 600: checked through flash_nsplit)."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from oracle import cpu_ref as O
from tests import t5_ref as T
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu

BAR = T.BAR16
FAR = 1e-1
SHAPES = ((31, 31), (129, 200), (300, 300), (160, 131), (1, 70), (130, 600))      # (q_len, kv_len); the last one splits its KV
SPLIT_SHAPE = (130, 600)
RADII = (1, 40, 128)
PARITY_RADIUS = {(31, 31): 8, (129, 200): 128, (300, 300): 40, (160, 131): 128, (1, 70): 16, (130, 600): 128}


def _bits(x, dtype) -> np.ndarray:
    x = np.ascontiguousarray(x, np.float32)
    return O.f32_to_bf16_bits(x) if dtype == "bf16" else x.astype(np.float16).view(np.uint16)


def _dev_bits(words, dtype):
    from pygpukit_amd.core import from_numpy

    words = np.ascontiguousarray(words, np.uint16)
    return from_numpy(words if dtype == "bf16" else words.view(np.float16))


def _host_bits(a) -> np.ndarray:
    h = a.to_numpy()
    return h if h.dtype == np.uint16 else h.view(np.uint16)


def _values(words, dtype) -> np.ndarray:
    return O.bf16_bits_to_f32(words) if dtype == "bf16" else words.view(np.float16).astype(np.float32)


def _dev(a):
    from pygpukit_amd.core import from_numpy

    return from_numpy(np.ascontiguousarray(a))


def _d0s(radius):
    return sorted({d for d in (0, 1, -1, 37, -radius + 1, radius - 1) if -radius < d < radius})


def _flash_nsplit(nqt, hq, kv_len, cus):
    """csrc/attn_plan.h flash_nsplit."""
    nsplit = 1
    while nsplit < 4 and nqt * hq * nsplit < 2 * cus and -(-kv_len // 64) >= 4 * (nsplit * 2):
        nsplit *= 2
    return nsplit


def _require_split(hq, q_len, kv_len):
    from pygpukit_amd.core.device import get_device_info

    cus = get_device_info().multiprocessor_count
    if _flash_nsplit(-(-q_len // 128), hq, kv_len, cus) < 2:
        pytest.skip(f"a device of {cus} CUs runs {hq} heads of {q_len} / {kv_len} in one KV run")


@functools.lru_cache(maxsize=None)
def _qkv(hq, hkv, q_len, kv_len, d, dtype, unit_scale, seed=5):
    """16-bit words (or float32 arrays for dtype "f32") of random Q / K / V; unit_scale: Q and K at D^-1/4 (see the header)."""
    rng = np.random.default_rng(seed + 7 * q_len + kv_len + d)
    s = d ** -0.25 if unit_scale else 1.0
    q = (rng.standard_normal((hq, q_len, d)) * s).astype(np.float32)
    k = (rng.standard_normal((hkv, kv_len, d)) * s).astype(np.float32)
    v = rng.standard_normal((hkv, kv_len, d)).astype(np.float32)
    if dtype == "f32":
        return q, k, v
    return tuple(_bits(x, dtype) for x in (q, k, v))


def _run(q, k, v, table, dtype, scale=0.0):
    from pygpukit_amd.ops.nn import sdpa_relbias

    if dtype == "f32":
        return sdpa_relbias(_dev(q), _dev(k), _dev(v), _dev(table.astype(np.float32)), scale).to_numpy()
    return _host_bits(sdpa_relbias(_dev_bits(q, dtype), _dev_bits(k, dtype), _dev_bits(v, dtype), _dev(table.astype(np.float32)), scale))


# ---- exact key selection -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("q_len,kv_len", SHAPES)
def test_one_delta_selects_one_key_bit_for_bit(q_len, kv_len, d, dtype):
    from pygpukit_amd.ops.nn import relbias_plan

    hq = 2
    if (q_len, kv_len) == SPLIT_SHAPE:
        _require_split(hq, q_len, kv_len)
    assert relbias_plan(d, 128, "bfloat16" if dtype == "bf16" else "float16") == "relbias_flash"
    q, k, v = _qkv(hq, hq, q_len, kv_len, d, dtype, False)
    checked = 0
    for radius in RADII:
        for d0 in _d0s(radius):
            rows = np.array([i for i in range(q_len) if 0 <= i + d0 < kv_len], np.int64)
            if rows.size == 0:
                continue
            table = np.full((hq, 2 * radius + 1), -1e4, np.float32)
            table[:, d0 + radius] = 0.0
            got = _run(q, k, v, table, dtype)
            want = v[:, rows + d0]
            bad = np.argwhere((got[:, rows] != want).any(axis=-1))
            assert bad.size == 0, (f"radius {radius}, d0 {d0}: {len(bad)} of {hq * rows.size} rows differ from V[i + d0]; first (head, row) "
                                   f"{(int(bad[0][0]), int(rows[bad[0][1]]))}")
            checked += rows.size
    assert checked > 0


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("q_len,kv_len,radius", [(129, 200, 40), (129, 200, 128), (300, 300, 40), (130, 600, 40), (130, 600, 128)])
def test_clamped_edge_selects_every_key_at_or_beyond_the_radius(q_len, kv_len, radius, d, dtype):
    """Table 0 only at delta <= -R, Q = 0, V small integers in one binade [4, 8): row i >= R is the exact mean of keys 0..i - R."""
    hq = 2
    if (q_len, kv_len) == SPLIT_SHAPE:
        _require_split(hq, q_len, kv_len)
    rng = np.random.default_rng(radius + q_len)
    vi = rng.integers(4, 8, (hq, kv_len, d)).astype(np.float32)
    q = np.zeros((hq, q_len, d), np.float32)
    k = rng.standard_normal((hq, kv_len, d)).astype(np.float32)
    table = np.full((hq, 2 * radius + 1), -1e4, np.float32)
    table[:, 0] = 0.0
    got = _run(_bits(q, dtype), _bits(k, dtype), _bits(vi, dtype), table, dtype)
    rows = [i for i in range(q_len) if i - radius >= 0]
    assert rows
    csum = np.cumsum(vi.astype(np.float64), axis=1)
    worst = 0
    for i in rows:
        n = min(i - radius, kv_len - 1) + 1
        want = _bits(csum[:, n - 1] / n, dtype).astype(np.int64)
        worst = max(worst, int(np.abs(got[:, i].astype(np.int64) - want).max()))
    print(f"clamped edge q {q_len} kv {kv_len} R {radius} D {d} {dtype}: worst distance {worst} 16-bit ulp over {len(rows)} rows")
    assert worst <= 1


# ---- numerical parity --------------------------------------------------------------------------------------------------

def _table(hq, radius, seed=11):
    """Random, asymmetric in delta, a few units in size, different for every head."""
    rng = np.random.default_rng(seed + radius)
    return (rng.standard_normal((hq, 2 * radius + 1)) * 2.0 + np.linspace(-1.5, 1.5, 2 * radius + 1)[None, :]).astype(np.float32)


@pytest.mark.parametrize("hq,hkv", [(3, 3), (4, 2)])
@pytest.mark.parametrize("q_len,kv_len", SHAPES)
def test_flash_parity_with_the_float64_restatement(q_len, kv_len, hq, hkv):
    radius = PARITY_RADIUS[(q_len, kv_len)]
    table = _table(hq, radius)
    for d in (64, 128):
        for dtype in ("bf16", "f16"):
            for scale in (1.0, 0.0):
                q, k, v = _qkv(hq, hkv, q_len, kv_len, d, dtype, scale == 1.0)
                ref = T.attention_relbias(_values(q, dtype), _values(k, dtype), _values(v, dtype), table, scale)
                got = _values(_run(q, k, v, table, dtype, scale), dtype)
                e = rel_err(got, ref)
                print(f"sdpa_relbias flash {dtype} D {d} heads {hq}/{hkv} q {q_len} kv {kv_len} R {radius} scale {scale or 'default'}: rel_err {e:.3e}")
                assert np.isfinite(got).all() and e <= BAR


@pytest.mark.parametrize("d", [64, 80, 256])
@pytest.mark.parametrize("q_len,kv_len", [(31, 31), (129, 200), (160, 131), (1, 70)])
def test_rows_kernel_parity_float32(q_len, kv_len, d):
    from pygpukit_amd.ops.nn import relbias_plan

    assert relbias_plan(d, 128, "float32") == "relbias_rows"
    hq, hkv, radius = 4, 2, PARITY_RADIUS[(q_len, kv_len)]
    table = _table(hq, radius)
    for scale in (1.0, 0.0):
        q, k, v = _qkv(hq, hkv, q_len, kv_len, d, "f32", scale == 1.0)
        ref64 = T.attention_relbias(q, k, v, table, scale)
        ref32 = T.attention_relbias(q, k, v, table, scale, dtype=np.float32)
        bar = T.f32_bar(ref32, ref64)
        got = _run(q, k, v, table, "f32", scale)
        e = rel_err(got, ref64)
        print(f"sdpa_relbias rows f32 D {d} q {q_len} kv {kv_len} scale {scale or 'default'}: rel_err {e:.3e}, rel_err(ref32, ref64) "
              f"{rel_err(ref32, ref64):.3e}, bar {bar:.3e}")
        assert np.isfinite(got).all() and e <= bar


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_rows_kernel_takes_other_head_dims_and_unaligned_buffers(dtype):
    from pygpukit_amd.core.array import GPUArray
    from pygpukit_amd.ops.nn import relbias_plan, sdpa_relbias

    name = "bfloat16" if dtype == "bf16" else "float16"
    assert relbias_plan(80, 128, name) == "relbias_rows" and relbias_plan(64, 128, name, aligned=False) == "relbias_rows"
    assert relbias_plan(64, 2000, name) == "relbias_rows"
    hq, hkv, q_len, kv_len = 4, 2, 129, 200
    table = _table(hq, 128)
    for d, shift in ((80, 0), (64, 1)):       # shift: every buffer starts one element past a 16-byte boundary
        q, k, v = _qkv(hq, hkv, q_len, kv_len, d, dtype, False)
        ref = T.attention_relbias(_values(q, dtype), _values(k, dtype), _values(v, dtype), table)
        bufs = []
        for words in (q, k, v):
            flat = np.zeros(words.size + shift, np.uint16)
            flat[shift:] = words.ravel()
            bufs.append(_dev_bits(flat, dtype)._view(shift, words.shape))
        out_buf = GPUArray((hq * q_len * d + shift,), bufs[0].dtype)
        out = out_buf._view(shift, (hq, q_len, d))
        sdpa_relbias(bufs[0], bufs[1], bufs[2], _dev(table), out=out)
        e = rel_err(_values(_host_bits(out), dtype), ref)
        print(f"sdpa_relbias rows {dtype} D {d} shift {shift}: rel_err {e:.3e}")
        assert e <= BAR


# ---- behaviour ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_bias_is_applied_with_the_right_sign_and_to_query_heads(dtype):
    hq, hkv, q_len, kv_len, d, radius = 4, 2, 129, 200, 64, 128
    table = _table(hq, radius)
    q, k, v = _qkv(hq, hkv, q_len, kv_len, d, dtype, False)
    vals = (lambda x: x) if dtype == "f32" else (lambda x: _values(x, dtype))
    ref = T.attention_relbias(vals(q), vals(k), vals(v), table)
    got = vals(_run(q, k, v, table, dtype))
    wrong = {"zero table": np.zeros_like(table), "reversed along delta": table[:, ::-1], "heads permuted": table[[1, 2, 3, 0]]}
    assert rel_err(got, ref) <= BAR
    for name, t in wrong.items():
        e = rel_err(got, T.attention_relbias(vals(q), vals(k), vals(v), t))
        print(f"sdpa_relbias {dtype}: rel_err against the {name} oracle {e:.3e}")
        assert e >= FAR


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("d", [64, 128])
def test_strided_call_is_bit_identical_to_the_contiguous_one(d, dtype):
    from pygpukit_amd.core.array import GPUArray
    from pygpukit_amd.ops.nn import sdpa_relbias_strided

    h, s, radius = 3, 200, 128
    table = _table(h, radius)
    q, k, v = _qkv(h, h, s, s, d, dtype, False)
    want = _run(q, k, v, table, dtype)
    # [S, 3 H D]: q | k | v per row, as a fused projection leaves them
    packed = np.concatenate([x.transpose(1, 0, 2).reshape(s, h * d) for x in (q, k, v)], axis=1)
    buf = _dev_bits(packed, dtype)
    rest = buf.size - 2 * h * d
    out = GPUArray((s, h * d), buf.dtype)
    sdpa_relbias_strided(buf, buf._view(h * d, (rest,)), buf._view(2 * h * d, (rest,)), _dev(table), out, h, h, s, s, d, (d, 3 * h * d),
                         (d, 3 * h * d), (d, h * d))
    got = _host_bits(out).reshape(s, h, d).transpose(1, 0, 2)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("q_len,kv_len", [(129, 200), (300, 300), (130, 600)])
def test_zero_table_is_bit_identical_to_sdpa_noncausal(q_len, kv_len, dtype):
    from pygpukit_amd.ops.nn import sdpa_noncausal

    hq, hkv = 4, 2
    for d in (64, 128):
        q, k, v = _qkv(hq, hkv, q_len, kv_len, d, dtype, False)
        want = _host_bits(sdpa_noncausal(_dev_bits(q, dtype), _dev_bits(k, dtype), _dev_bits(v, dtype)))
        got = _run(q, k, v, np.zeros((hq, 2 * 40 + 1), np.float32), dtype)
        assert np.array_equal(got, want)
