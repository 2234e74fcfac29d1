"""FP8 (OCP e4m3) KV cache on the GPU: the quantising cache writer and the scale helper byte for byte against tests/kv_fp8_ref.py,
the split-KV decode over the 8-bit cache against the float64 oracle ON THE SAME CODES (so the bar measures the kernel's arithmetic,
not quantisation), exact checks of the two scales and of the masking, and the operator-surface model on an fp8 cache.

Bars: rel_err <= 1e-2 for bf16 / f16 against the float64 oracle, what the sdpa_causal and window parity tests hold these dtypes to
(the oracle rounded to bf16 is ~1.7e-3 from itself at these shapes)."""

from __future__ import annotations

import functools
from unittest import mock

import numpy as np
import pytest

from oracle import cpu_ref as O
from tests import attn_stair_ref as S
from tests import kv_fp8_ref as R
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu

TABLE = O.fp8_e4m3_table()
NAN_CODE, SENTINEL = 0x7F, 0xA5


def _dev(x, dtype):
    from pygpukit_amd.core import from_numpy

    w = S.to_words(x, dtype)
    return from_numpy(np.ascontiguousarray(w.view(np.float16) if dtype == "f16" else w))


def _host(a, dtype):
    h = a.to_numpy()
    return S.from_words(h if h.dtype == np.uint16 else h.view(np.uint16), dtype).astype(np.float64)


def _f32(a):
    from pygpukit_amd.core import from_numpy

    return from_numpy(np.ascontiguousarray(a, np.float32))


# ---- writer and scale helper: exact bytes -------------------------------------------------------------------------------------------
W_SCALES = np.array([0.375, 1.9], np.float32)       # 0.375 = 3 / 8: every tie of head 0 below divides back to the exact midpoint


def _writer_input(seq, d, dtype):
    """[seq, 2, d]: random values of which ~1 in 5 lie beyond +-448 scale; row 0 of head 0 starts with +-0, values beyond the range,
    and +- every third midpoint between neighbouring codes (subnormal codes included) times 0.375, all exact in bf16 and f16."""
    rng = np.random.default_rng(seq * 1000 + d)
    x = rng.standard_normal((seq, 2, d)) * 350.0 * W_SCALES[None, :, None]
    x[:, 1, ::7] *= 2.0 ** -9                       # subnormal-range quotients (below 2 ** -6) in head 1
    mids = ((TABLE[:0x7E] + TABLE[1:0x7F]) / 2)[::3].astype(np.float64)
    special = np.concatenate([[0.0, -0.0, 449.0, -449.0, 2e4, -2e4], mids[:29], -mids[13:42]]) * 0.375
    x[0, 0, :len(special)] = special
    return S.round_to(x, dtype)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("seq", [1, 5])
@pytest.mark.parametrize("form", ["host", "ptr"])
def test_writer_bytes(form, seq, d, dtype):
    from pygpukit_amd.core import from_numpy
    from pygpukit_amd.ops.nn import kv_cache_prefill_gqa_fp8, kv_cache_update_gqa_fp8_ptr

    x = _writer_input(seq, d, dtype)
    assert np.isin(np.abs(x[0, 0, 6:64] / np.float32(0.375)), (TABLE[:0x7E] + TABLE[1:0x7F]) / 2).all()      # the ties survive the rounding to dtype
    cache = from_numpy(np.full((2, 8, d), SENTINEL, np.uint8))
    want = np.full((2, 8, d), SENTINEL, np.uint8)
    want[:, 2:2 + seq] = R.quantise(x, W_SCALES).transpose(1, 0, 2)
    assert not np.isin(want[:, 2:2 + seq], (0x7F, 0xFF)).any() and (want == 0x7E).any() and (want == 0x80).any()
    if form == "host":
        kv_cache_prefill_gqa_fp8(_dev(x, dtype), cache, _f32(W_SCALES), 2)
    else:
        kv_cache_update_gqa_fp8_ptr(_dev(x, dtype), cache, _f32(W_SCALES), from_numpy(np.array([2], np.int32)))
    np.testing.assert_array_equal(cache.to_numpy(), want)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_absmax_scales(dtype):
    from pygpukit_amd.ops.nn import kv_fp8_scales

    x = S.round_to(np.random.default_rng(5).standard_normal((37, 3, 64)) * 3.0, dtype)
    x[:, 1] = 0.0
    np.testing.assert_array_equal(kv_fp8_scales(_dev(x, dtype), 3).to_numpy(), R.absmax_scales(x))


# ---- decode parity ------------------------------------------------------------------------------------------------------------------
def _chunk(max_seq, step):
    nsplit = max(1, -(-max_seq // 256))
    return -(-(-(-max_seq // nsplit)) // step) * step


@functools.lru_cache(maxsize=None)
def _decode_case(hq, hkv, d, max_seq, dtype):
    rng = np.random.default_rng(hq * 100 + hkv + d + max_seq)
    q = S.round_to(rng.standard_normal((hq, 1, d)), dtype)
    k, v = (rng.standard_normal((hkv, max_seq, d)) for _ in range(2))
    ks, vs = (np.abs(a).max(axis=(1, 2)).astype(np.float32) / np.float32(224.0) for a in (k, v))
    kc, vc = R.quantise(k, ks, head_axis=0), R.quantise(v, vs, head_axis=0)
    exact = O.sdpa_causal_fixed_cache(q.astype(np.float64), np.repeat(k, hq // hkv, 0), np.repeat(v, hq // hkv, 0), max_seq)
    print(f"fp8 cache against the unquantised cache, ctx {max_seq}: rel_err {rel_err(R.decode(q, kc, vc, ks, vs, max_seq), exact):.3e}")
    for a in (q, kc, vc, ks, vs):
        a.setflags(write=False)
    return q, kc, vc, ks, vs


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("max_seq", [64, 600])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("hq,hkv", [(8, 2), (4, 2), (3, 3)])
def test_decode_against_the_oracle(hq, hkv, d, max_seq, dtype):
    """Rows at and beyond ctx hold the NaN code in K and V.  The _ptr form is ONE call sequence, only the device length rewritten."""
    from pygpukit_amd.core import from_numpy
    from pygpukit_amd.ops.nn import sdpa_causal_fixed_cache_fp8, sdpa_causal_fixed_cache_fp8_ptr, sdpa_kv_fp8_plan

    q, kc, vc, ks, vs = _decode_case(hq, hkv, d, max_seq, dtype)
    step, chunk = (32 if d == 128 else 64), _chunk(max_seq, 32 if d == 128 else 64)
    assert sdpa_kv_fp8_plan(hq, hkv, d, max_seq, "bfloat16" if dtype == "bf16" else "float16") == ("kv_fp8_split", 1 if max_seq == 64 else 3)
    qd, ksd, vsd, ctx_buf = _dev(q, dtype), _f32(ks), _f32(vs), from_numpy(np.zeros(1, np.int32))
    for ctx in sorted({c for c in (1, step - 1, step, step + 1, chunk - 1, chunk, chunk + 1, max_seq - 1, max_seq) if 1 <= c <= max_seq}):
        kd, vd = (from_numpy(np.concatenate([a[:, :ctx], np.full_like(a[:, ctx:], NAN_CODE)], axis=1)) for a in (kc, vc))
        ref = R.decode(q, kc, vc, ks, vs, ctx)
        out_h, out_p = (from_numpy(np.full((hq, 1, d), 0x7FC0 if dtype == "bf16" else 0x7E00, np.uint16).view(np.float16 if dtype == "f16" else np.uint16))
                        for _ in range(2))
        sdpa_causal_fixed_cache_fp8(qd, kd, vd, ksd, vsd, out_h, ctx)
        ctx_buf.copy_from_numpy(np.array([ctx], np.int32))
        sdpa_causal_fixed_cache_fp8_ptr(qd, kd, vd, ksd, vsd, out_p, ctx_buf, max_seq)
        for name, out in (("host", out_h), ("ptr", out_p)):
            got = _host(out, dtype)
            assert np.isfinite(got).all(), f"{name} form, ctx {ctx}: not finite"
            e = rel_err(got, ref)
            print(f"{name} ctx {ctx}: rel_err {e:.3e}")
            assert e <= 1e-2, f"{name} form, ctx {ctx}, cache {max_seq}: rel_err {e:.3e}"


# ---- scales and masking, exactly -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("d", [64, 128])
def test_scales_and_mask_exactly(d, dtype):
    """K codes 0: a uniform softmax over ctx = 256 rows of a 600-row cache (three chunks).  V[r, h, j] = 4 where (r + j + h) % 8 <= j % 8,
    else 0: the mean is (j % 8 + 1) / 2 exactly, times v_scale.  Rows from ctx on hold the NaN code."""
    from pygpukit_amd.core import from_numpy
    from pygpukit_amd.ops.nn import sdpa_causal_fixed_cache_fp8

    hq, hkv, rows, ctx = 8, 2, 600, 256
    r, h, j = np.ogrid[:ctx, :hkv, :d]
    vals = np.where((r + j + h) % 8 <= j % 8, 4.0, 0.0)
    kc, vc = np.full((hkv, rows, d), NAN_CODE, np.uint8), np.full((hkv, rows, d), NAN_CODE, np.uint8)
    kc[:, :ctx], vc[:, :ctx] = 0, R.quantise(vals, [1.0, 1.0]).transpose(1, 0, 2)
    mean = np.broadcast_to((np.arange(d) % 8 + 1) / 2.0, (hq, 1, d))
    q = _dev(np.random.default_rng(d).standard_normal((hq, 1, d)), dtype)
    for k_scale, v_scale in ((1.0, 0.5), (3.7, 0.5), (1.0, 1.0)):
        out = from_numpy(np.zeros((hq, 1, d), np.float16 if dtype == "f16" else np.uint16))
        sdpa_causal_fixed_cache_fp8(q, from_numpy(kc), from_numpy(vc), _f32([k_scale] * hkv), _f32([v_scale] * hkv), out, ctx)
        np.testing.assert_array_equal(_host(out, dtype), mean * v_scale, err_msg=f"k_scale {k_scale}, v_scale {v_scale}")


# ---- the operator-surface model ------------------------------------------------------------------------------------------------------
MODEL = dict(vocab_size=512, hidden_size=128, num_layers=2, num_heads=4, num_kv_heads=2, head_dim=64, intermediate_size=256,
             rope_theta=1e4, norm_eps=1e-5)
EMBED_GAIN = 16
_plain_sdpa = O.sdpa_causal


class _Fp8CacheRefAttention(O.RefAttention):
    """The oracle's attention whose single-token steps read K and V through quantise / dequantise with `scales` (per KV head); a
    prompt attends its own fresh K / V, as the model's does."""

    def __call__(self, x, position_ids, past_kv=None, use_cache=False):
        if x.shape[0] > 1:
            return super().__call__(x, position_ids, past_kv, use_cache)
        ks, vs = (np.repeat(s, self.num_kv_groups) for s in self.scales)        # the oracle hands sdpa_causal GQA-expanded [Hq, kv, D]

        def through_cache(q, k, v):
            return _plain_sdpa(q, R.dequantise(R.quantise(k, ks, head_axis=0), ks).astype(q.dtype),
                               R.dequantise(R.quantise(v, vs, head_axis=0), vs).astype(q.dtype))

        with mock.patch.object(O, "sdpa_causal", through_cache):
            return super().__call__(x, position_ids, past_kv, use_cache)


@pytest.mark.parametrize("kv_scales", ["unit", "prompt"])
def test_model_on_an_fp8_cache_against_the_oracle(kv_scales):
    """12 prompt tokens, then 6 steps through the fp8 caches, the oracle's ids fed to both.  The oracle's steps read its K / V through
    quantise / dequantise with the scales the model holds; every logits row is held to the model tests' bar, 1e-2.

    The embedding is EMBED_GAIN = 16 times the other matrices' std 0.02 (a power of two: exact in bf16, and the tied head only scales
    the logits).  Chosen on the CPU oracle alone: the quantiser is a step function, so the oracle's OWN logits move when its K / V
    change by what separates any 16-bit model from it (6e-3, step 0 of the unquantised model) before quantise - by 2.1e-2 / 6.1e-3 /
    3.4e-3 at gains 1 / 8 / 16, because at gain 1 a layer's attention output is 3.5 times the residual stream it is added to.  16 is
    the smallest power of two that keeps this wobble of the reference under half the bar.  What that costs: the logits here see a
    wiring error (scales, rows, positions: an attention output off by tens of per cent), not a few per cent of attention error -
    that is test_decode_against_the_oracle's and test_writer_bytes' job.  On an MI355X the cached steps are 3.8e-3 .. 4.8e-3 from the oracle
    (at gain 1: 1.74e-2 / 1.59e-2, the reference's wobble)."""
    from pygpukit_amd.llm.synthetic import build_model_from_weights

    weights = O.make_qwen3_weights(MODEL, seed=38, bf16=True, std=0.02)
    weights["embed"] = weights["embed"] * np.float32(EMBED_GAIN)
    prompt = [int(t) for t in np.random.default_rng(38).integers(0, 512, 12)]
    model = build_model_from_weights(MODEL, weights, max_pos=64)
    with pytest.raises(NotImplementedError, match="sliding-window"):
        build_model_from_weights(MODEL, weights, max_pos=64, sliding_window=8).init_fixed_cache(40, "bfloat16", kv_dtype="fp8")
    got = model.generate(prompt, max_new_tokens=3, temperature=0.0, top_k=0, top_p=1.0, use_cache=True, kv_dtype="fp8", kv_scales=kv_scales)
    assert len(got) == 15 and got[:12] == prompt
    model.init_fixed_cache(40, "bfloat16", kv_dtype="fp8", kv_scales=kv_scales)
    assert all(b.attn._k_cache.to_numpy().dtype == np.uint8 and b.attn._k_cache.shape == (2, 40, 64) for b in model.blocks)
    logits = model.prefill_fixed_cache(prompt)
    with pytest.raises(NotImplementedError, match="one prompt chunk from position 0"):
        model._decode_step_fixed_cache_batch(prompt[:3], 12, 15)
    ref = O.build_qwen3_ref(MODEL, weights, max_pos=64)
    for rb, b in zip(ref.blocks, model.blocks):
        rb.attn.__class__, rb.attn.scales = _Fp8CacheRefAttention, (b.attn._k_scale.to_numpy(), b.attn._v_scale.to_numpy())
        assert (rb.attn.scales[0] == 1.0).all() == (kv_scales == "unit")
    hidden, past = ref(prompt, use_cache=True)
    tokens = list(prompt)
    for step in range(7):
        want = np.asarray(ref.get_logits(hidden), np.float64)[-1]
        e = rel_err(_host(logits, "bf16")[-1], want)
        print(f"{kv_scales} step {step}: rel_err {e:.3e}")
        assert e <= 1e-2, f"step {step}: rel_err {e:.3e}"
        tokens.append(int(want.argmax()))
        hidden, past = ref([tokens[-1]], past_key_values=past, use_cache=True)
        logits = model.get_logits(model._decode_step_fixed_cache(tokens[-1], len(tokens) - 1, len(tokens)))
