"""The FLUX row kernels on the GPU (csrc/ops_flux.hip).  flux_qk_norm_rope on both dispatch leaves, element by element against the
float64 oracle of tests/flux_ref.py evaluated on the inputs as the device holds them, with every element outside Q and K checked
bit for bit; flux_gelu_pack against the gelu op bit for bit; flux_unpack_latents against the reference's record; flow_euler_step
against float64.

Bars of flux_qk_norm_rope, per element (the convention of test_dit_ops_gpu.py):
  float32:  FACTOR32 * yard, yard = the largest per-element error |ref32 - ref64| of the np.float32 restatement of the same formula
            on the same case (a property of float32 and of the case, not of the kernel); never above CAP32 = 1e-4 (the data is O(1)).
  16-bit:   one ulp of the output dtype at |ref| plus the float32 term above.
FACTOR32 is the smallest power of two at least twice the worst ratio max|gpu - ref64| / yard measured on an MI355X over every
float32 case of this file: MEASURED_RATIO below, printed again by every test (run with -s).

Every case uses a random GENERAL [S, D] table (the two elements of a pair carry different values), so a kernel that assumed the
repeat-interleaved tables of get_rope_frequencies would fail everywhere."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from tests import flux_ref as R
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

g15 = load_golden("g15_flux.npz")
MEASURED_RATIO = 2.397   # worst max|gpu - ref64| / yard over the float32 cases, measured on an MI355X (scalar kernel, head_dim 32;
                         # next: vector kernel head_dim 64 2.351, scalar head_dim 6 2.080, 72 1.966, vector 128 1.815, one element
                         # off alignment 1.520); twice it is 4.794
FACTOR32 = 8.0
CAP32 = 1e-4
DTYPES = ["f32", "bf16", "f16"]
NAMES = {"f32": "float32", "bf16": "bfloat16", "f16": "float16"}
SHAPES = [(1, 1, 0), (1, 11, 5), (2, 11, 5), (2, 7, 7), (1, 70, 1)]        # (batch, seq, split)
EPS = 1e-6


def _dev(a, dtype):
    """Upload values already rounded to `dtype`."""
    from pygpukit_amd.core import from_numpy

    return from_numpy(R.to_words(a, dtype))


def _words(a):
    return np.ascontiguousarray(a.to_numpy())


def _draw(shape, dtype, seed, std=1.0, mean=0.0):
    out = R.round_to(mean + std * np.random.default_rng(seed).standard_normal(shape), dtype)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _tables(rows, D, seed=77):
    rng = np.random.default_rng(seed + D)
    cos, sin = (rng.uniform(-1, 1, (rows, D)).astype(np.float32) for _ in range(2))
    return cos, sin


def _bar(dtype, ref64, ref32):
    yard = float(np.abs(ref32.astype(np.float64) - ref64).max())
    term32 = min(FACTOR32 * yard, CAP32)
    return yard, term32, (term32 if dtype == "f32" else R.ULP[dtype] * np.abs(ref64) + term32)


class _Case:
    """One call: Q and K inside a fused [rows, 3 H D] buffer ("fused"), or in two buffers whose rows carry a gap after every head
    and a tail ("separate"); offset shifts the first element off the buffer's start."""

    def __init__(self, dtype, B, S, split, H, D, layout, w_dtype, offset=0, seed=0):
        self.dtype, self.B, self.S, self.split, self.H, self.D = dtype, B, S, split, H, D
        rows = B * S
        if layout == "fused":
            self.head_stride, self.row_stride, self.k_off = D, 3 * H * D, H * D
            self.host = [np.array(_draw((offset + rows * self.row_stride + 8,), dtype, seed + 1))]
        else:
            self.head_stride = D + 8
            self.row_stride, self.k_off = H * self.head_stride + 16, None
            self.host = [np.array(_draw((offset + rows * self.row_stride + 8,), dtype, seed + 1 + i)) for i in range(2)]
        self.offset = offset
        wd = dtype if w_dtype == "row" else "f32"
        self.w_dtype = wd
        self.w = [_draw((D,), wd, seed + 10 + i, 0.3, 1.0) for i in range(4)]            # wq_a, wk_a, wq_b, wk_b
        self.cos, self.sin = _tables(max(S, 2 * 11), D)

    def _index(self):
        r, h, j = np.meshgrid(np.arange(self.B * self.S), np.arange(self.H), np.arange(self.D), indexing="ij")
        return self.offset + r * self.row_stride + h * self.head_stride + j

    def qk(self, buffers):
        """-> Q, K [B, S, H, D] out of the flat buffers."""
        idx = self._index()
        q = buffers[0][idx]
        k = buffers[0][idx + self.k_off] if self.k_off is not None else buffers[1][idx]
        return (a.reshape(self.B, self.S, self.H, self.D) for a in (q, k))

    def refs(self, dtype, **wrong):
        q, k = self.qk(self.host)
        return (R.qk_norm_rope(q, self.w[0], self.w[2], self.split, self.cos, self.sin, EPS, dtype, **wrong),
                R.qk_norm_rope(k, self.w[1], self.w[3], self.split, self.cos, self.sin, EPS, dtype, **wrong))

    def run(self):
        from pygpukit_amd.diffusion.ops import flux_qk_norm_rope

        bufs = [_dev(h, self.dtype) for h in self.host]
        before = [_words(b) for b in bufs]
        q = bufs[0]._view(self.offset, (bufs[0].size - self.offset,))
        kb, ko = (bufs[0], self.offset + self.k_off) if self.k_off is not None else (bufs[1], self.offset)
        k = kb._view(ko, (kb.size - ko,))
        need_a, need_b = self.split > 0, self.split < self.S
        w = [_dev(x, self.w_dtype) for x in self.w]
        flux_qk_norm_rope(q, k, _dev(self.cos, "f32"), _dev(self.sin, "f32"), w[0] if need_a else None, w[1] if need_a else None,
                          batch=self.B, seq=self.S, heads=self.H, head_dim=self.D, row_stride=self.row_stride,
                          head_stride=self.head_stride, split=self.split, wq_b=w[2] if need_b else None, wk_b=w[3] if need_b else None,
                          eps=EPS)
        after = [_words(b) for b in bufs]
        touched = [np.zeros(b.shape, bool) for b in before]
        idx = self._index()
        touched[0][idx] = True
        (touched[0] if self.k_off is not None else touched[1])[idx + (self.k_off or 0)] = True
        for b, a, t in zip(before, after, touched):
            assert np.array_equal(b[~t].view(np.uint8), a[~t].view(np.uint8)), "an element outside Q and K changed"
            assert (~t).sum() >= 8
        return [R.from_words(a, self.dtype).astype(np.float64) for a in after]

    def check(self, name, got):
        """-> the worst float32 ratio max|gpu - ref64| / yard of this case (0 for the 16-bit dtypes)."""
        worst_ratio = 0.0
        for label, g, r64, r32 in zip("QK", self.qk(got), self.refs(np.float64), self.refs(np.float32)):
            yard, term32, bar = _bar(self.dtype, r64, r32)
            err = np.abs(g - r64)
            assert np.isfinite(g).all() and yard > 0 and term32 <= CAP32
            over = err > bar
            assert not over.any(), (f"{name} {label}: {int(over.sum())} of {over.size} elements over the bar, worst err / bar "
                                    f"{float((err / bar).max()):.3f}, yard {yard:.3e}")
            if self.dtype == "f32":
                worst_ratio = max(worst_ratio, float(err.max() / yard))
        return worst_ratio

    def misses(self, got, **wrong):
        """-> the fraction of Q and K elements that are over the bar of the WRONG oracle, and the worst err / bar."""
        frac, worst = [], 0.0
        for g, r64, r32 in zip(self.qk(got), self.refs(np.float64, **wrong), self.refs(np.float32, **wrong)):
            _, _, bar = _bar(self.dtype, r64, r32)
            err = np.abs(g - r64)
            frac.append(float((err > bar).mean()))
            worst = max(worst, float((err / bar).max()))
        return min(frac), worst


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [64, 128, 32, 72, 6])
def test_qk_norm_rope_on_every_shape_layout_and_weight_dtype(D, dtype):
    """head_dim 64 / 128 take the vector kernel, the others the scalar one; (1, 70, 1) with 3 heads is 420 heads: no multiple of
    the 32 / 16 / 8 heads a vector block owns nor of the 4 the scalar block owns; B = 2 repeats the table per element."""
    from pygpukit_amd.diffusion.ops import flux_qk_norm_rope_plan

    want = "flux_qk_norm_rope_vec" if D in (64, 128) else "flux_qk_norm_rope_scalar"
    assert flux_qk_norm_rope_plan(D, NAMES[dtype]) == want
    ratio, n = 0.0, 0
    for H in (1, 3):
        for B, S, split in SHAPES:
            for layout in ("fused", "separate"):
                for w_dtype in ("row", "f32"):
                    case = _Case(dtype, B, S, split, H, D, layout, w_dtype, seed=1000 * D + 100 * H + 10 * S + B)
                    ratio = max(ratio, case.check(f"D={D} H={H} B={B} S={S} split={split} {layout} w={w_dtype} {dtype}", case.run()))
                    n += 1
    print(f"flux_qk_norm_rope {want} D={D} {dtype}: {n} cases pass" + (f", worst ratio {ratio:.3f}" if dtype == "f32" else "") +
          f" (MEASURED_RATIO {MEASURED_RATIO}, FACTOR32 {FACTOR32})")
    assert n == 40 and ratio <= FACTOR32


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [64, 128])
def test_a_view_off_16_byte_alignment_takes_the_scalar_kernel(D, dtype):
    from pygpukit_amd.diffusion.ops import flux_qk_norm_rope_plan

    assert flux_qk_norm_rope_plan(D, NAMES[dtype], aligned=False) == "flux_qk_norm_rope_scalar"
    ratio = 0.0
    for layout in ("fused", "separate"):
        case = _Case(dtype, 2, 11, 5, 3, D, layout, "row", offset=1, seed=31 * D)
        ratio = max(ratio, case.check(f"misaligned D={D} {layout} {dtype}", case.run()))
    print(f"flux_qk_norm_rope one element off alignment D={D} {dtype}: pass" + (f", worst ratio {ratio:.3f}" if dtype == "f32" else "") +
          f" (MEASURED_RATIO {MEASURED_RATIO})")
    assert ratio <= FACTOR32


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("D", [64, 72])
@pytest.mark.parametrize("control", ["swapped_weights", "rotate_half", "global_row"])
def test_wrong_formulas_miss_the_bar(control, D, dtype):
    """Negative controls on both kernels: the device result passes the right oracle's bar and misses, by a wide margin, the bar
    of an oracle with the text / image norm weights swapped, with the rotate-half pairing, or with the table indexed by the global
    row b * S + p at B = 2."""
    case = _Case(dtype, 2, 11, 5, 3, D, "fused", "row", seed=500 + D)
    got = case.run()
    case.check(f"{control} D={D} {dtype}", got)
    wrong = {"swapped_weights": dict(swap_weights=True), "rotate_half": dict(pairing="half"), "global_row": dict(global_row=True)}[control]
    frac, worst = case.misses(got, **wrong)
    print(f"{control} D={D} {dtype}: {frac:.2f} of the elements over the wrong oracle's bar, worst err / bar {worst:.1f}")
    # global_row leaves batch element 0 right: half of the elements at the most can miss
    assert frac > (0.3 if control == "global_row" else 0.6) and worst > 20


def test_qk_norm_rope_rejects_what_it_cannot_run():
    from pygpukit_amd.diffusion.ops import flux_qk_norm_rope

    q = _dev(_draw((4 * 3 * 64,), "f32", 1), "f32")
    w, cos = _dev(_draw((64,), "f32", 2), "f32"), _dev(_tables(22, 64)[0], "f32")
    kw = dict(batch=1, seq=4, heads=1, head_dim=64, row_stride=192)
    k = q._view(64, (q.size - 64,))
    with pytest.raises(ValueError, match="even"):
        flux_qk_norm_rope(q, k, cos, cos, w, w, **dict(kw, head_dim=7))
    with pytest.raises(ValueError, match="split"):
        flux_qk_norm_rope(q, k, cos, cos, w, w, split=5, **kw)
    with pytest.raises(ValueError, match="wq_b"):
        flux_qk_norm_rope(q, k, cos, cos, w, w, split=2, **kw)
    with pytest.raises(ValueError, match="rows"):
        flux_qk_norm_rope(q, k, cos, cos, w, w, **dict(kw, seq=5))
    with pytest.raises(ValueError, match="float32"):
        flux_qk_norm_rope(q, k, _dev(_draw((4, 64), "bf16", 3), "bf16"), cos, w, w, **kw)
    with pytest.raises(ValueError, match="wq"):
        flux_qk_norm_rope(_dev(_draw((768,), "f16", 1), "f16"), _dev(_draw((768,), "f16", 1), "f16"), cos, cos,
                          _dev(_draw((64,), "bf16", 2), "bf16"), w, **kw)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cols,width,column", [(5, 32, 48, 16), (5, 30, 47, 5), (3, 32, 41, 8), (520, 4096, 4104, 8)])
def test_gelu_pack_is_the_gelu_op_bit_for_bit(rows, cols, width, column, dtype):
    """(5, 32, 48, 16): whole 16-byte vectors; 30 columns: no multiple of the vector width; width 41: a row stride off the vector
    width; 520 x 4096: more vectors than one pass of the grid, so the grid-stride loop runs."""
    from pygpukit_amd.diffusion.ops import flux_gelu_pack
    from pygpukit_amd.ops.nn.activation import gelu

    x = _dev(_draw((rows, cols), dtype, rows + cols, 2.0), dtype)
    dest_host = R.to_words(_draw((rows, width), dtype, width), dtype)
    dest = _dev(_draw((rows, width), dtype, width), dtype)
    out = flux_gelu_pack(x, dest, column=column)
    assert out is dest
    got, want = _words(dest), _words(gelu(x))
    assert np.array_equal(np.ascontiguousarray(got[:, column:column + cols]).view(np.uint8), want.view(np.uint8))
    keep = np.ones(width, bool)
    keep[column:column + cols] = False
    assert np.array_equal(np.ascontiguousarray(got[:, keep]).view(np.uint8), np.ascontiguousarray(dest_host[:, keep]).view(np.uint8))
    if rows <= 5:
        ref = R.gelu_tanh(R.from_words(_words(x), dtype).astype(np.float64))
        assert np.abs(R.from_words(want, dtype) - ref).max() <= 2 * R.ULP[dtype] * np.abs(ref).max()
    with pytest.raises(ValueError, match="columns"):
        flux_gelu_pack(x, dest, column=width - cols + 1)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_unpack_latents_is_the_reference_move(dtype):
    from pygpukit_amd.diffusion.models.flux import FluxPipeline
    from pygpukit_amd.diffusion.ops import flux_unpack_latents

    x = R.round_to(g15["unpack_in"], dtype)
    want = R.to_words(R.unpack_latents(x, 2, 3), dtype)
    got = flux_unpack_latents(_dev(x, dtype), 2, 3)
    assert got.shape == (2, 16, 4, 6)
    assert np.array_equal(_words(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8))
    if dtype == "f32":
        np.testing.assert_array_equal(_words(got), g15["unpack_out"])
        # pack_latents is the inverse move
        np.testing.assert_array_equal(_words(FluxPipeline.pack_latents(got)), g15["unpack_in"])
    with pytest.raises(ValueError, match="expects"):
        flux_unpack_latents(_dev(x, dtype), 3, 3)


@pytest.mark.parametrize("dtype", DTYPES)
def test_flow_euler_step_within_one_float32_ulp(dtype):
    """600 001 elements: more than one pass of the grid.  sample + dt * v in float64 on the float32 step; the fused multiply-add
    rounds once, so the result is within half an ulp - the bar is one."""
    from pygpukit_amd.diffusion.models.flux import FlowMatchEulerScheduler
    from pygpukit_amd.diffusion.ops import flow_euler_step

    n = 600_001
    sample, v = np.array(_draw((n,), "f32", 5)), _draw((n,), dtype, 6)
    dt = np.float32(-0.25) + np.float32(2 ** -20)
    s = _dev(sample, "f32")
    assert flow_euler_step(s, _dev(v, dtype), float(dt)) is s
    ref = sample.astype(np.float64) + np.float64(dt) * v.astype(np.float64)
    err = np.abs(_words(s).astype(np.float64) - ref)
    assert (err <= np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)).all()
    # the scheduler's device branch is this kernel with dt = sigma_next - sigma, and advances the step index
    sched = FlowMatchEulerScheduler()
    sched.set_timesteps(4)
    x = _dev(g15["sched_sample"], "f32")
    for i, t in enumerate(sched.timesteps):
        assert sched.step(_dev(R.round_to(g15["sched_velocity"][i], dtype), dtype), t, x) is x and sched.step_index == i + 1
    ref = g15["sched_sample"].astype(np.float64)
    for i in range(4):
        ref = ref + np.float64(sched.sigmas[i + 1] - sched.sigmas[i]) * R.round_to(g15["sched_velocity"][i], dtype).astype(np.float64)
    assert np.abs(_words(x) - ref).max() <= 4 * 2.0 ** -23 * np.abs(ref).max()
    with pytest.raises(ValueError, match="float32"):
        flow_euler_step(_dev(v, dtype), _dev(v, dtype), 0.1) if dtype != "f32" else flow_euler_step(s, _dev(v[:5], dtype), 0.1)
