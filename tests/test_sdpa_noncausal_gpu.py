"""sdpa_noncausal / sdpa_noncausal_strided on the GPU: the FlashFull policy of the second-generation flash kernel (every q_len),
its KV-split + merge path, and the non-causal fallback kernel (float32, PYGPUKIT_FLASH_ATTENTION=0).

Numerical: rel_err <= 1e-2 for bf16 / f16 (the project's bar) against the float64 oracle on the rounded inputs; the float32
fallback is held to rtol = atol = 2e-5, the bar tests/test_gpu_ops.py holds the causal float32 path to.

Exact visibility: with Q = 0 every score is exactly 0 and every probability exactly 1 / kv_len; with V zero except row j* = 1
every output element must be 1 / kv_len.  The kernels compute 1 * fl32(1 / l) and round once: the bar is (u + 2^-22) / kv_len
with u the output rounding (2^-8 bf16, 2^-11 f16, 0 float32) and 2^-22 for the fp32 reciprocal.  A dropped key j* gives 0, a
causal mask 1 / (i + 1) or 0 on early rows, one padded key 1 / (kv_len + 1) - all beyond the bar (tests/test_whisper_cpu.py).
kv_len 65 and 200 are four KV tiles at most, which the launcher never splits, so the split path also runs kv_len = 1000 (four runs
of 256, 256, 256 and 232 keys at these head counts; nothing is asserted about the count).  There a partial output is rounded
to the dtype before the merge kernel rounds the result: two roundings, bar (2 u + 2^-21) / kv_len.

Unchanged neighbours: sdpa_causal shares flash_fwd_kernel's template.  The SHA-256 values below are of its raw output on three
second-generation shapes (one of them split), recorded on an MI355X from a build of the parent commit - the commit before the
FlashFull policy existed - with the inputs of _neighbour_inputs."""

from __future__ import annotations

import functools
import hashlib

import numpy as np
import pytest

from tests import whisper_ref as R
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu

U = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}
SPLIT_SHAPE = R.ATTN_SHAPES[4]


def _dev(x, dtype):
    from pygpukit_amd.core import from_numpy

    w = R.to_words(x, dtype)
    return from_numpy(np.ascontiguousarray(w.view(np.float16) if dtype == "f16" else w))


def _words(a, dtype):
    h = a.to_numpy()
    return h if dtype == "f32" or h.dtype == np.uint16 else h.view(np.uint16)


def _host(a, dtype):
    return R.from_words(_words(a, dtype), dtype).astype(np.float64)


def _nan_out(shape, dtype):
    from pygpukit_amd.core import from_numpy

    if dtype == "f32":
        return from_numpy(np.full(shape, np.nan, np.float32))
    w = np.full(shape, 0x7FC0 if dtype == "bf16" else 0x7E00, np.uint16)
    return from_numpy(w.view(np.float16) if dtype == "f16" else w)


@functools.lru_cache(maxsize=None)
def _case(shape, dtype):
    q, k, v = (R.round_to(a, dtype) for a in R.make_attn_case(shape))
    ref = R.sdpa_noncausal(q, k, v)
    for a in (q, k, v, ref):
        a.setflags(write=False)
    return q, k, v, ref


def _run(q, k, v, dtype, out=None):
    from pygpukit_amd.ops.nn import sdpa_noncausal

    return sdpa_noncausal(_dev(q, dtype), _dev(k, dtype), _dev(v, dtype), out=out)


# ---- numerical --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("shape", R.ATTN_SHAPES, ids=str)
def test_flash_kernel_against_the_oracle(shape, dtype):
    q, k, v, ref = _case(shape, dtype)
    out = _nan_out(ref.shape, dtype)
    assert _run(q, k, v, dtype, out=out) is out
    got = _host(out, dtype)
    e = rel_err(got, ref)
    print(f"sdpa_noncausal {shape} {dtype}: rel_err {e:.3e}, max |err| {np.abs(got - ref).max():.3e}")
    assert np.isfinite(got).all() and e <= 1e-2


@pytest.mark.parametrize("shape", R.ATTN_SHAPES[:4] + ((2, 1, 9, 77, 40),), ids=str)
def test_float32_fallback_against_the_oracle(shape):
    q, k, v, ref = _case(shape, "f32")
    got = _host(_run(q, k, v, "f32"), "f32")
    np.testing.assert_allclose(got, ref, rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_forced_fallback_and_odd_head_dim_in_16_bit(dtype, monkeypatch):
    q, k, v, ref = _case((2, 1, 9, 77, 40), dtype)                   # head_dim 40: no MFMA kernel
    assert rel_err(_host(_run(q, k, v, dtype), dtype), ref) <= 1e-2
    monkeypatch.setenv("PYGPUKIT_FLASH_ATTENTION", "0")
    q, k, v, ref = _case(R.ATTN_SHAPES[1], dtype)
    assert rel_err(_host(_run(q, k, v, dtype), dtype), ref) <= 1e-2


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
def test_strided_form_reads_the_fused_projection_in_place(dtype):
    """One [S, 3 H D] buffer, q | k | v per row, as the encoder's fused QKV GEMM leaves it; out [S, H D]."""
    from pygpukit_amd.ops.nn import sdpa_noncausal_strided

    H, S, D = 2, 150, 64
    buf = R.round_to(np.random.default_rng(77).standard_normal((S, 3 * H * D)).astype(np.float32), dtype)
    q, k, v = (buf[:, i * H * D:(i + 1) * H * D].reshape(S, H, D).transpose(1, 0, 2) for i in range(3))
    ref = R.sdpa_noncausal(q, k, v).transpose(1, 0, 2).reshape(S, H * D)
    qkv = _dev(buf, dtype)
    rest = qkv.size - 2 * H * D
    out = _nan_out((S, H * D), dtype)
    sdpa_noncausal_strided(qkv, qkv._view(H * D, (rest,)), qkv._view(2 * H * D, (rest,)), out, H, H, S, S, D, (D, 3 * H * D),
                           (D, 3 * H * D), (D, H * D))
    got = _host(out, dtype)
    if dtype == "f32":
        np.testing.assert_allclose(got, ref, rtol=2e-5, atol=2e-5)
    else:
        assert np.isfinite(got).all() and rel_err(got, ref) <= 1e-2


# ---- exact visibility -------------------------------------------------------------------------------------------------
def _visibility(hq, hkv, q_len, kv_len, d, dtype, roundings):
    _, k, _ = R.make_attn_case((hq, hkv, q_len, kv_len, d))
    q = np.zeros((hq, q_len, d), np.float32)
    bar = (roundings * U[dtype] + roundings * 2.0 ** -22) / kv_len
    for j_star in (0, 63, 64, kv_len - 1):
        v = np.zeros((hkv, kv_len, d), np.float32)
        v[:, j_star] = 1.0
        got = _host(_run(q, R.round_to(k, dtype), v, dtype, out=_nan_out((hq, q_len, d), dtype)), dtype)
        err = np.abs(got - 1.0 / kv_len)
        assert np.all(err <= bar), (f"kv_len {kv_len}, j* {j_star}, {dtype}: {int((err > bar).sum())} of {err.size} elements are not 1 / kv_len; "
                                    f"values seen {np.unique(got)[:6]}")


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("kv_len", [65, 200])
def test_every_key_is_visible_to_every_row_flash(kv_len, dtype):
    _visibility(2, 2, 70, kv_len, 64, dtype, 1)
    _visibility(4, 2, 130, kv_len, 128, dtype, 1)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("kv_len", [65, 200, 1000])
def test_every_key_is_visible_to_every_row_split(kv_len, dtype):
    """The split shape's head counts; kv_len 1000 is the length at which the launcher cuts the keys into runs."""
    _visibility(2, 1, 130, kv_len, 64, dtype, 2 if kv_len == 1000 else 1)


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("kv_len", [65, 200])
def test_every_key_is_visible_to_every_row_fallback(kv_len, dtype, monkeypatch):
    monkeypatch.setenv("PYGPUKIT_FLASH_ATTENTION", "0")
    _visibility(2, 2, 70, kv_len, 64, dtype, 1)


# ---- poison beyond the lengths ------------------------------------------------------------------------------------------
def _strided_run(q, k, v, q_len, kv_len, dtype):
    """q [rows >= q_len, Hq D], k / v [rows >= kv_len, Hkv D] host arrays -> raw words of out [q rows, Hq D] (NaN-filled before)."""
    from pygpukit_amd.ops.nn import sdpa_noncausal_strided

    d = 64
    hq, hkv = q.shape[1] // d, k.shape[1] // d
    out = _nan_out(q.shape, dtype)
    sdpa_noncausal_strided(_dev(q, dtype), _dev(k, dtype), _dev(v, dtype), out, hq, hkv, q_len, kv_len, d, (d, hq * d), (d, hkv * d), (d, hq * d))
    return _words(out, dtype)


@pytest.mark.parametrize("path", ["flash", "split", "fallback"])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_rows_beyond_the_lengths_are_never_read(path, dtype, monkeypatch):
    """64 extra K / V rows (K = 100, V = 1e4) and 64 extra Q rows (1e4) behind the lengths passed: the result equals the run
    on clean buffers bit for bit, and the output rows beyond q_len stay untouched."""
    if path == "fallback":
        monkeypatch.setenv("PYGPUKIT_FLASH_ATTENTION", "0")
    hq, hkv, q_len, kv_len, d = (2, 1, 130, 1000, 64) if path == "split" else (2, 2, 70, 200, 64)
    rng = np.random.default_rng(5)
    q = R.round_to(rng.standard_normal((q_len, hq * d)).astype(np.float32), dtype)
    k, v = (R.round_to(rng.standard_normal((kv_len, hkv * d)).astype(np.float32), dtype) for _ in range(2))
    clean = _strided_run(q, k, v, q_len, kv_len, dtype)
    qp = np.concatenate([q, np.full((64, hq * d), 1e4, np.float32)])
    kp = np.concatenate([k, np.full((64, hkv * d), 100.0, np.float32)])
    vp = np.concatenate([v, np.full((64, hkv * d), 1e4, np.float32)])
    got = _strided_run(qp, kp, vp, q_len, kv_len, dtype)
    np.testing.assert_array_equal(got[:q_len], clean)
    np.testing.assert_array_equal(got[q_len:], 0x7FC0 if dtype == "bf16" else 0x7E00)
    ref = R.sdpa_noncausal(*(a.reshape(a.shape[0], -1, d).transpose(1, 0, 2) for a in (q, k, v)))
    assert rel_err(R.from_words(clean, dtype).reshape(q_len, hq, d).transpose(1, 0, 2), ref) <= 1e-2


# ---- unchanged neighbours ---------------------------------------------------------------------------------------------
PARENT_SHA256 = {
    (4, 2, 200, 333, 64, "bf16"): "ac63850114af2003dd5769df449d98b30628e91c2f8f1a368354bbfe2a6ab6cc",
    (4, 2, 200, 333, 128, "f16"): "a5cd745ff95815124412586ca44d6b21ce4a054fe863b212e75034463e99238f",
    (2, 1, 130, 1000, 64, "bf16"): "16d4abd16cd65b8f922e14bc2e72a9ad9fcb30f34b922ef0d9e60d30644c130d",
}


def _neighbour_inputs(case):
    hq, hkv, q_len, kv_len, d, dtype = case
    rng = np.random.default_rng(1234)
    return [R.round_to(rng.standard_normal(s).astype(np.float32), dtype) for s in ((hq, q_len, d), (hkv, kv_len, d), (hkv, kv_len, d))]


@pytest.mark.parametrize("case", PARENT_SHA256, ids=str)
def test_sdpa_causal_output_is_what_the_parent_build_gave(case):
    from pygpukit_amd.ops.nn import sdpa_causal

    out = sdpa_causal(*(_dev(a, case[5]) for a in _neighbour_inputs(case))).to_numpy()
    assert hashlib.sha256(np.ascontiguousarray(out).view(np.uint8).tobytes()).hexdigest() == PARENT_SHA256[case]
