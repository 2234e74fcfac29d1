"""pygpukit_amd.diffusion.ops on the GPU: the fused AdaLN row kernel on both dispatch leaves, element by element against the float64
oracle of tests/dit_ref.py evaluated on the inputs as the device holds them; patchify / unpatchify exactly; the 4-D attention
wrappers, the timestep embedding and the modulation projection.

Bars of the row kernel, per element:
  float32:  FACTOR32 * yard, yard = the largest per-element error |ref32 - ref64| of a np.float32 restatement of the same formula
            on the same case, computed here (a property of float32 and of the case, not of the kernel); never above CAP32 = 1e-4
            (the data is O(1)).
  16-bit:   one ulp of the output dtype at |ref| (2^-7 |ref| for bfloat16, 2^-10 |ref| for float16; round-to-nearest itself costs
            half of that) plus the float32 term above.
FACTOR32 is the smallest power of two at least twice the worst ratio max|gpu - ref64| / yard measured on an MI355X over every
float32 case of this file: MEASURED_RATIO below, printed again by every test (run with -s)."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from tests import dit_ref as R
from tests.conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

g13 = load_golden("g13_pixart.npz")
MEASURED_RATIO = 2.012   # worst max|gpu - ref64| / yard over the float32 cases, measured on an MI355X (adaln on the recorded case;
                         # next: layer_norm_simple 1.801, adaln_zero 1.645, no_gate D=100 1.464); twice it is 4.024
FACTOR32 = 8.0
CAP32 = 1e-4
DTYPES = ["f32", "bf16", "f16"]
TOP = {"f32": 2048, "bf16": 4096, "f16": 4096}       # the largest feature count of the wave-per-row kernel
VEC = {"f32": 4, "bf16": 8, "f16": 8}                # elements per 16-byte vector


def _pk(dtype):
    from pygpukit_amd.core.dtypes import bfloat16, float16, float32

    return {"f32": float32, "bf16": bfloat16, "f16": float16}[dtype]


def _dev(a, dtype):
    """Upload values already rounded to `dtype`."""
    from pygpukit_amd.core import from_numpy

    return from_numpy(R.to_words(a, dtype))


def _host(a, dtype):
    return R.from_words(a.to_numpy(), dtype).astype(np.float64)


def _draw(shape, dtype, seed, std=1.0):
    out = R.round_to(std * np.random.default_rng(seed).standard_normal(shape), dtype)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _case(B, N, D, dtype, vec_dtype=None):
    """value, residual [B, N, D] and gate / scale / shift [B, D], as the device holds them."""
    vd = vec_dtype or dtype
    seed = 7 * D + 3 * N + B
    return (_draw((B, N, D), dtype, seed), _draw((B, N, D), dtype, seed + 1), _draw((B, D), vd, seed + 2, 0.5),
            _draw((B, D), vd, seed + 3, 0.5), _draw((B, D), vd, seed + 4, 0.5))


def _check(name, dtype, got, ref64, ref32):
    """got: float64 view of the device result; ref64 / ref32: the oracle in float64 and in float32 on the same inputs."""
    yard = float(np.abs(ref32.astype(np.float64) - ref64).max())
    term32 = min(FACTOR32 * yard, CAP32)
    err = np.abs(got - ref64)
    bar = term32 if dtype == "f32" else R.ULP[dtype] * np.abs(ref64) + term32
    worst = float((err / np.maximum(bar, 1e-300)).max())
    ratio = float(err.max() / yard) if yard > 0 else 0.0
    print(f"{name} {dtype}: max err {err.max():.3e}, yard {yard:.3e}" + (f", ratio {ratio:.3f}" if dtype == "f32" else "") +
          f", worst err / bar {worst:.3f}")
    # 16-bit inputs can make the float32 restatement exact (a product of two bfloat16 values fits float32): yard == 0 is then
    # legitimate and the ulp term alone is the bar
    assert np.isfinite(got).all() and (yard > 0 or dtype != "f32") and term32 <= CAP32
    assert (err <= bar).all(), f"{name} {dtype}: {int((err > bar).sum())} elements over the bar, worst err / bar {worst:.3f}"


def _fused_refs(x, res, gate, scale, shift, eps, norm=True):
    return [R.fused(x, res, gate, scale, shift, eps, norm, dt) for dt in (np.float64, np.float32)]


SHAPE_CASES = [(B, N, D) for (B, N) in ((2, 5), (1, 1)) for D in (8, 72, 1152, "top", "top+vec", 100, 7)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,N,D", SHAPE_CASES)
def test_gated_residual_adaln_on_every_leaf(B, N, D, dtype):
    """B=2, N=5: ten rows in blocks of four waves - the second block holds rows of both batch elements, the third is partial."""
    from pygpukit_amd.diffusion.ops import adaln_plan, gated_residual_adaln

    D = {"top": TOP[dtype], "top+vec": TOP[dtype] + VEC[dtype]}.get(D, D)
    want = "adaln_wave" if D % VEC[dtype] == 0 and D <= TOP[dtype] else "adaln_block"
    assert adaln_plan(D, _pk(dtype)) == want
    assert want == {8: "adaln_wave", 72: "adaln_wave", 1152: "adaln_wave", 7: "adaln_block", 100: "adaln_wave" if dtype == "f32" else "adaln_block"}.get(D, want)
    x, res, gate, scale, shift = _case(B, N, D, dtype)
    s, y = gated_residual_adaln(_dev(x, dtype), _dev(res, dtype), _dev(gate, dtype), _dev(scale, dtype), _dev(shift, dtype), 1e-6)
    assert s.shape == y.shape == (B, N, D) and s.dtype == y.dtype == _pk(dtype)
    (s64, y64), (s32, y32) = _fused_refs(x, res, (None, gate), (None, scale), (None, shift), 1e-6)
    _check(f"sum [{B},{N},{D}] {want}", dtype, _host(s, dtype), s64, s32)
    _check(f"y   [{B},{N},{D}] {want}", dtype, _host(y, dtype), y64, y32)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_view_off_16_byte_alignment_takes_the_block_kernel(dtype):
    from pygpukit_amd.core.array import GPUArray
    from pygpukit_amd.diffusion.ops import adaln_plan, gated_residual_adaln

    B, N, D = 2, 5, 72
    x, res, gate, scale, shift = _case(B, N, D, dtype)
    buf = GPUArray((B * N * D + 8,), _pk(dtype))
    buf.copy_from_numpy(R.to_words(np.concatenate([np.zeros(1, np.float32), x.ravel(), np.zeros(7, np.float32)]), dtype))
    xv = buf._view(1, (B, N, D))
    assert xv.data_ptr() % 16 != 0 and adaln_plan(D, _pk(dtype), aligned=False) == "adaln_block"
    s, y = gated_residual_adaln(xv, _dev(res, dtype), _dev(gate, dtype), _dev(scale, dtype), _dev(shift, dtype), 1e-6)
    (s64, y64), (s32, y32) = _fused_refs(x, res, (None, gate), (None, scale), (None, shift), 1e-6)
    _check("misaligned sum", dtype, _host(s, dtype), s64, s32)
    _check("misaligned y", dtype, _host(y, dtype), y64, y32)


@pytest.mark.parametrize("D", [72, 100])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("form", ["no_gate", "no_residual", "no_norm", "table_only", "vector_only", "stride0", "table+strided"])
def test_absent_arguments(form, dtype, D):
    """Every combination the model uses.  table+strided is PixArt's: rows of a [6, D] table and of a [B, 6, D] projection."""
    from pygpukit_amd.diffusion.ops import Modulation, gated_residual_adaln

    B, N = 2, 5
    x, res, gate, scale, shift = _case(B, N, D, dtype)
    table = _draw((6, D), dtype, 99 + D, 0.5)
    cond = _draw((B, 6, D), dtype, 98 + D, 0.5)
    dx, dres = _dev(x, dtype), _dev(res, dtype)
    dg, dsc, dsh, dtab, dcond = (_dev(a, dtype) for a in (gate, scale, shift, table, cond))
    if form == "no_gate":
        got = gated_residual_adaln(dx, dres, None, dsc, dsh, 1e-6)
        refs = _fused_refs(x, res, None, (None, scale), (None, shift), 1e-6)
    elif form == "no_residual":
        got = gated_residual_adaln(dx, None, None, dsc, dsh, 1e-6)
        assert got[0] is None
        refs = _fused_refs(x, None, None, (None, scale), (None, shift), 1e-6)
    elif form == "no_norm":
        got = gated_residual_adaln(dx, dres, dg, dsc, dsh, 1e-6, norm=False)
        refs = _fused_refs(x, res, (None, gate), (None, scale), (None, shift), 1e-6, norm=False)
    elif form == "table_only":
        got = gated_residual_adaln(dx, dres, Modulation(dtab, table_offset=2 * D), Modulation(dtab, table_offset=D), dtab._view(0, (D,)), 1e-6)
        refs = _fused_refs(x, res, (table[2], None), (table[1], None), (table[0], None), 1e-6)
    elif form == "vector_only":
        got = gated_residual_adaln(dx, dres, dg, None, dsh, 1e-6)
        refs = _fused_refs(x, res, (None, gate), None, (None, shift), 1e-6)
    elif form == "stride0":
        got = gated_residual_adaln(dx, dres, Modulation(vector=dg, stride=0), Modulation(vector=dsc, vector_offset=D, stride=0), dsh, 1e-6)
        refs = _fused_refs(x, res, (None, gate[0]), (None, scale[1]), (None, shift), 1e-6)
    else:
        def m(k):
            return Modulation(dtab, dcond, table_offset=k * D, vector_offset=k * D, stride=6 * D)

        got = gated_residual_adaln(dx, dres, m(5), m(1), m(0), 1e-6)
        refs = _fused_refs(x, res, (table[5], cond[:, 5]), (table[1], cond[:, 1]), (table[0], cond[:, 0]), 1e-6)
    (s64, y64), (s32, y32) = refs
    if got[0] is not None:
        _check(f"{form} D={D} sum", dtype, _host(got[0], dtype), s64, s32)
    _check(f"{form} D={D} y", dtype, _host(got[1], dtype), y64, y32)


@pytest.mark.parametrize("D", [1152, 100])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_float32_vectors_under_16_bit_rows(dtype, D):
    from pygpukit_amd.diffusion.ops import Modulation, gated_residual_adaln

    B, N = 2, 5
    x, res, _, _, _ = _case(B, N, D, dtype)
    table, cond = _draw((6, D), "f32", 199 + D, 0.5), _draw((B, 6, D), "f32", 198 + D, 0.5)
    dtab, dcond = _dev(table, "f32"), _dev(cond, "f32")

    def m(k):
        return Modulation(dtab, dcond, table_offset=k * D, vector_offset=k * D, stride=6 * D)

    s, y = gated_residual_adaln(_dev(x, dtype), _dev(res, dtype), m(2), m(4), m(3), 1e-6)
    (s64, y64), (s32, y32) = _fused_refs(x, res, (table[2], cond[:, 2]), (table[4], cond[:, 4]), (table[3], cond[:, 3]), 1e-6)
    _check(f"f32 vectors D={D} sum", dtype, _host(s, dtype), s64, s32)
    _check(f"f32 vectors D={D} y", dtype, _host(y, dtype), y64, y32)
    with pytest.raises(ValueError, match="dtype"):
        gated_residual_adaln(_dev(x, dtype), _dev(res, dtype), m(2), _dev(cond[:, 0], dtype), m(3), 1e-6)


@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_named_ops(dtype):
    """adaln / adaln_zero on the reference's recorded case (float32: also against its recorded outputs), and the native-only ops."""
    from pygpukit_amd.diffusion.ops import adaln, adaln_zero, gated_residual, layer_norm_simple, modulate

    x, res, scale, shift, gate = (R.round_to(g13[k], dtype) for k in ("ada_x", "ada_res", "ada_scale", "ada_shift", "ada_gate"))
    dx, dres, dsc, dsh, dg = (_dev(a, dtype) for a in (x, res, scale, shift, gate))
    got = _host(adaln(dx, dsc, dsh), dtype)
    _check("adaln", dtype, got, R.adaln(x, scale, shift), R.adaln(x, scale, shift, dtype=np.float32))
    got_zero = _host(adaln_zero(dx, dsc, dsh, dg, dres), dtype)
    _check("adaln_zero", dtype, got_zero, R.adaln_zero(x, scale, shift, gate, res), R.adaln_zero(x, scale, shift, gate, res, dtype=np.float32))
    if dtype == "f32":
        print(f"vs the reference's recorded outputs: adaln {rel_err(got, g13['ada_out']):.3e}, adaln_zero {rel_err(got_zero, g13['ada_zero_out']):.3e}")
        assert rel_err(got, g13["ada_out"]) < 5e-7 and rel_err(got_zero, g13["ada_zero_out"]) < 5e-7
    refs = _fused_refs(x, None, None, None, None, 1e-5)
    _check("layer_norm_simple", dtype, _host(layer_norm_simple(dx), dtype), refs[0][1], refs[1][1])
    refs = _fused_refs(x, None, None, (None, scale), (None, shift), 0.0, norm=False)
    _check("modulate", dtype, _host(modulate(dx, dsc, dsh), dtype), refs[0][1], refs[1][1])
    refs = _fused_refs(x, res, (None, gate), None, None, 0.0, norm=False)
    _check("gated_residual", dtype, _host(gated_residual(dres, dg, dx), dtype), refs[0][0], refs[1][0])
    out = adaln(dx, dsc, dsh, out=dx)
    assert out is dx
    np.testing.assert_array_equal(_host(dx, dtype), got)


@pytest.mark.parametrize("D", [72, 1152, 7, 2052])
def test_fused_is_bit_identical_to_gated_residual_then_adaln_in_float32(D):
    from pygpukit_amd.diffusion.ops import adaln, gated_residual, gated_residual_adaln

    x, res, gate, scale, shift = (_dev(a, "f32") for a in _case(2, 5, D, "f32"))
    s, y = gated_residual_adaln(x, res, gate, scale, shift, 1e-6)
    s2 = gated_residual(res, gate, x)
    y2 = adaln(s2, scale, shift, 1e-6)
    np.testing.assert_array_equal(s.to_numpy(), s2.to_numpy())
    np.testing.assert_array_equal(y.to_numpy(), y2.to_numpy())


@pytest.mark.parametrize("D", [72, 100])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_in_place_forms(dtype, D):
    """sum_out is residual and y is x, on the wave kernel and on the block kernel, against the out-of-place call bit for bit."""
    from pygpukit_amd.diffusion.ops import gated_residual_adaln

    x, res, gate, scale, shift = _case(2, 5, D, dtype)
    dg, dsc, dsh = (_dev(a, dtype) for a in (gate, scale, shift))
    s, y = gated_residual_adaln(_dev(x, dtype), _dev(res, dtype), dg, dsc, dsh, 1e-6)
    dx, dres = _dev(x, dtype), _dev(res, dtype)
    s2, y2 = gated_residual_adaln(dx, dres, dg, dsc, dsh, 1e-6, sum_out=dres, out=dx)
    assert s2 is dres and y2 is dx
    np.testing.assert_array_equal(dres.to_numpy(), s.to_numpy())
    np.testing.assert_array_equal(dx.to_numpy(), y.to_numpy())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("p", [1, 2, 4])
def test_patchify_and_unpatchify_are_exact(p, dtype):
    from pygpukit_amd import _hip
    from pygpukit_amd.diffusion.ops import patchify, unpatchify

    B, C, H, W = 2, 3, 8, 12
    x = _draw((B, C, H, W), dtype, 5 + p)
    got = patchify(_dev(x, dtype), p)
    assert got.shape == (B * (H // p) * (W // p), C * p * p)
    np.testing.assert_array_equal(R.from_words(got.to_numpy(), dtype), R.patchify(x, p))
    Co = 5
    t = _draw((B * (H // p) * (W // p), p * p * Co), dtype, 6 + p)
    back = unpatchify(_dev(t, dtype), B, Co, H, W, p)
    assert back.shape == (B, Co, H, W)
    np.testing.assert_array_equal(R.from_words(back.to_numpy(), dtype), R.unpatchify(t, B, Co, H, W, p))
    # the two column orders differ ((c, ph, pw) against (ph, pw, c)), so the round trip is the identity when p == 1 or C == 1
    # and the oracle's fixed permutation otherwise
    round_trip = R.from_words(unpatchify(got, B, C, H, W, p).to_numpy(), dtype)
    np.testing.assert_array_equal(round_trip, R.unpatchify(R.patchify(x, p), B, C, H, W, p))
    if p == 1:
        np.testing.assert_array_equal(round_trip, x)
    one = _draw((B, 1, H, W), dtype, 7 + p)
    np.testing.assert_array_equal(R.from_words(unpatchify(patchify(_dev(one, dtype), p), B, 1, H, W, p).to_numpy(), dtype), one)
    with pytest.raises(ValueError, match="multiples"):
        patchify(_dev(_draw((1, 1, 9, 12), dtype, 1), dtype), 2 if p == 1 else p)
    dx = _dev(x, dtype)
    with pytest.raises(_hip.PgkError, match="multiples of the patch size"):
        _hip.call("pgk_patchify", dx._p, got._p, B, C, H, W, 5, dx.dtype.code, None)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_attention_4d(dtype):
    """The reference's recorded case: [2, 3, 7, 16] queries on [2, 3, 5, 16] keys.  What is new here is the wrapper (the loop over
    the batch on views), not the attention kernels, which tests/test_whisper_gpu.py and test_attention_mask_gpu.py hold to 2e-6
    absolute in float32: a wrong batch or head offset moves the output by O(1), so rel_err <= 1e-5 in float32 and <= 1e-2, the
    project's bar, in the 16-bit dtypes decide it."""
    from pygpukit_amd.diffusion.ops import cross_attention, self_attention

    q, k, v = (R.round_to(g13[n], dtype) for n in ("ca_q", "ca_k", "ca_v"))
    ref = R.attention(q, k, v)
    out = cross_attention(_dev(q, dtype), _dev(k, dtype), _dev(v, dtype))
    assert out.shape == (2, 3, 7, 16) and out.dtype == _pk(dtype)
    e = rel_err(_host(out, dtype), ref)
    yard = rel_err(g13["ca_out"], R.attention(g13["ca_q"], g13["ca_k"], g13["ca_v"]))
    bar = 1e-5 if dtype == "f32" else 1e-2
    print(f"cross_attention {dtype}: rel_err {e:.3e}, rel_err(fixture, ref64) {yard:.3e}")
    assert e <= bar
    same = self_attention(_dev(k, dtype), _dev(k, dtype), _dev(v, dtype), 0.25)
    assert rel_err(_host(same, dtype), R.attention(k, k, v, 0.25)) <= bar
    with pytest.raises(NotImplementedError, match="mask"):
        cross_attention(_dev(q, dtype), _dev(k, dtype), _dev(v, dtype), mask=_dev(q, dtype))


def test_timestep_embedding_mlp_and_modulation():
    from pygpukit_amd.diffusion.ops import Modulation, adaln, modulation, sinusoidal_timestep_embedding, timestep_mlp

    emb = sinusoidal_timestep_embedding(g13["ts_t"], 64)
    np.testing.assert_array_equal(emb.to_numpy(), g13["ts_64"])
    np.testing.assert_array_equal(sinusoidal_timestep_embedding(_dev(g13["ts_t"], "f32"), 10, 1000.0).to_numpy(), g13["ts_10"])
    assert sinusoidal_timestep_embedding(g13["ts_t"], 64, dtype="bfloat16").dtype == _pk("bf16")
    rng = np.random.default_rng(3)
    w1, b1, w2, b2 = (rng.standard_normal(s).astype(np.float32) / 8 for s in ((48, 64), (48,), (72, 48), (72,)))
    got = timestep_mlp(emb, *(_dev(a, "f32") for a in (w1, b1, w2, b2))).to_numpy()
    e64 = g13["ts_64"].astype(np.float64)
    ref = R.silu(e64 @ w1.T.astype(np.float64) + b1) @ w2.T.astype(np.float64) + b2
    assert got.shape == (5, 72) and rel_err(got, ref) < 1e-5
    # modulation: one GEMM, the six vectors read in place
    cond = _draw((2, 72), "f32", 11)
    wm, bm = _draw((6 * 72, 72), "f32", 12, 0.1), _draw((6 * 72,), "f32", 13, 0.3)
    mods = modulation(_dev(cond, "f32"), _dev(wm, "f32"), _dev(bm, "f32"))
    assert len(mods) == 6 and all(isinstance(m, Modulation) for m in mods) and len({id(m.vector) for m in mods}) == 1
    proj = (cond.astype(np.float64) @ wm.T + bm).reshape(2, 6, 72)
    x = _case(2, 5, 72, "f32")[0]
    got = adaln(_dev(x, "f32"), mods[1], mods[0], 1e-6).to_numpy()
    assert rel_err(got, R.adaln(x, proj[:, 1], proj[:, 0], 1e-6)) < 1e-5
    one = modulation(_dev(cond[:1], "f32"), _dev(wm, "f32"), _dev(bm, "f32"))
    assert all(m.shape == (1, 72) and not m.owns_memory for m in one)
    assert rel_err(one[3].to_numpy(), proj[:1, 3]) < 1e-5
