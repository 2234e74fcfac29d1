"""Multi-head latent attention on the GPU against the float64 oracle tests/mla_ref.py.  Bar: rel_err <= 1e-2, what every decode parity
test here holds 16-bit attention to; the kernel's unavoidable roundings alone are under 2.6e-3 at every shape below (test_mla_cpu.py)."""

import numpy as np
import pytest

from tests import attn_stair_ref as S
from tests import mla_ref as R
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu

NAN = {"bf16": 0x7FC0, "f16": 0x7E00}
T = 32          # KV tile height of mla_decode_kernel


def _words(w, dtype):
    from pygpukit_amd.core import from_numpy

    return from_numpy(np.ascontiguousarray(w.view(np.float16) if dtype == "f16" else w))


def _dev(x, dtype="bf16"):
    return _words(S.to_words(x, dtype), dtype)


def _host(a, dtype):
    h = a.to_numpy()
    return S.from_words(h if h.dtype == np.uint16 else h.view(np.uint16), dtype).astype(np.float64)


def _chunk(q_len, heads, max_seq, dtype, ctx=None):
    from pygpukit_amd.ops.nn import sdpa_mla_plan

    chunks = sdpa_mla_plan(heads, q_len, max_seq, "bfloat16" if dtype == "bf16" else "float16")[2]
    return -(-(-(-(ctx or max_seq) // chunks)) // T) * T


def _run(q, cache, ctxs, dtype, scale):
    """Both forms at every context, NaN in rows >= ctx and in the output buffers; the _ptr form is ONE call sequence, only the device int rewritten."""
    from pygpukit_amd.core import from_numpy
    from pygpukit_amd.ops.nn import sdpa_mla_fixed_cache, sdpa_mla_fixed_cache_ptr

    qd, ctx_buf, cw = _dev(q, dtype), from_numpy(np.zeros(1, np.int32)), S.to_words(cache, dtype)
    for ctx in ctxs:
        cd = _words(np.concatenate([cw[:ctx], np.full_like(cw[ctx:], NAN[dtype])]), dtype)
        out_h, out_p = (_words(np.full(q.shape[:2] + (R.LATENT,), NAN[dtype], np.uint16), dtype) for _ in range(2))
        sdpa_mla_fixed_cache(qd, cd, out_h, ctx, scale)
        ctx_buf.copy_from_numpy(np.array([ctx], np.int32))
        sdpa_mla_fixed_cache_ptr(qd, cd, out_p, ctx_buf, scale)
        yield "host", ctx, _host(out_h, dtype)
        yield "ptr", ctx, _host(out_p, dtype)


def _check(q, cache, ctxs, dtype, scale=R.SCALE):
    for form, ctx, got in _run(q, cache, ctxs, dtype, scale):
        assert np.isfinite(got).all(), f"{form} form, ctx {ctx}: not finite"
        e = rel_err(got, R.op(q, cache, ctx, scale))
        print(f"{form} ctx {ctx}: rel_err {e:.3e}")
        assert e <= 1e-2, f"{form} form, ctx {ctx}: rel_err {e:.3e}"


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("q_len,heads,max_seq", R.DECODE_SHAPES)
def test_decode_against_the_oracle(q_len, heads, max_seq, dtype):
    chunk = _chunk(q_len, heads, max_seq, dtype)
    ctxs = sorted({c for c in (1, T - 1, T, T + 1, chunk - 1, chunk, chunk + 1, max_seq - 1, max_seq) if 1 <= c <= max_seq})
    _check(*R.case(q_len, heads, max_seq, dtype), ctxs, dtype)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("q_len,heads,max_seq", R.MULTI_SHAPES)
def test_several_query_rows(q_len, heads, max_seq, dtype):
    """The columns' limits on both sides of a tile edge (32, 576) and of a chunk edge (384: the live chunk length there is 128)."""
    edge = 384 + (q_len + 1) // 2
    assert _chunk(q_len, heads, max_seq, dtype, edge) == 128
    _check(*R.case(q_len, heads, max_seq, dtype), (q_len, T + (q_len + 1) // 2, edge, max_seq), dtype)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("gap", [64, 128])
@pytest.mark.parametrize("q_len,heads", [(5, 20), (1, 128)])
def test_mask_on_a_staircase(q_len, heads, gap, dtype):
    """Columns 0 / 1 of the cache hold r >> 4 and r & 15 and every query 16 g and g there, g = gap / scale: the score of row r is
    gap * r plus a few units of noise, so a query row's first INVISIBLE row beats all its visible ones by about `gap` and its last
    visible row carries its largest visible score - an off-by-one either way moves the output to another row (rel_err ~ 1.4).
    gap 64: the project's bar.  gap 128: every other exp2 is 0 in fp32, the output IS the last visible row's latent, bit for bit."""
    scale, max_seq = 0.125, 600
    q, cache = (np.array(a) for a in R.case(q_len, heads, max_seq, dtype))
    rows = np.arange(max_seq)
    cache[:, 0], cache[:, 1], q[..., 0], q[..., 1] = rows >> 4, rows & 15, 16 * gap / scale, gap / scale
    for form, ctx, got in _run(q, cache, (q_len, T, T + 1, 384 + (q_len + 1) // 2, max_seq), dtype, scale):
        want = np.repeat(cache[ctx - q_len:ctx, None, :R.LATENT], heads, axis=1)
        if gap == 128:
            np.testing.assert_array_equal(got, want, err_msg=f"{form} form, ctx {ctx}")
        else:
            assert np.isfinite(got).all() and rel_err(got, R.op(q, cache, ctx, scale)) <= 1e-2 and rel_err(got, want) <= 1e-2, (form, ctx)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("table", ["f32", "same"])
@pytest.mark.parametrize("seq", [1, 5])
@pytest.mark.parametrize("form", ["host", "ptr"])
def test_writer_bits(form, seq, table, dtype):
    """Rows 3 .. of a sentinel-filled cache are rmsnorm + rope_inplace + a copy on the same device arrays, bit for bit; nothing else is written."""
    from pygpukit_amd.core import from_numpy
    from pygpukit_amd.llm.layers.rope import precompute_freqs_cis
    from pygpukit_amd.ops.nn import mla_cache_write, mla_cache_write_ptr, rmsnorm, rope_inplace, rope_inplace_f32table

    rng, pos, rows = np.random.default_rng(seq), 3, 16
    kv_a, gamma = S.round_to(rng.standard_normal((seq, R.WIDTH)) * 3.0, dtype), S.round_to(1.0 + 0.2 * rng.standard_normal(R.LATENT), dtype)
    up = from_numpy if table == "f32" else (lambda a: _dev(a, dtype))
    cos, sin = (up(np.ascontiguousarray(t, np.float32)) for t in precompute_freqs_cis(R.ROPE, rows))
    cache = _words(np.full((rows, R.WIDTH), 0xA5A5, np.uint16), dtype)
    if form == "host":
        mla_cache_write(_dev(kv_a, dtype), _dev(gamma, dtype), cos, sin, cache, pos, 1e-6)
    else:
        mla_cache_write_ptr(_dev(kv_a, dtype), _dev(gamma, dtype), cos, sin, cache, from_numpy(np.array([pos], np.int32)), 1e-6)
    latent = rmsnorm(_dev(kv_a[:, :R.LATENT], dtype), _dev(gamma, dtype), 1e-6)
    kpe = _dev(kv_a[:, None, R.LATENT:], dtype)
    (rope_inplace_f32table if table == "f32" else rope_inplace)(kpe, kpe._view(0, (seq, 0, R.ROPE)), cos._view(pos * R.ROPE, (seq, R.ROPE)),
                                                                 sin._view(pos * R.ROPE, (seq, R.ROPE)))
    want = np.full((rows, R.WIDTH), 0xA5A5, np.uint16)
    want[pos:pos + seq, :R.LATENT], want[pos:pos + seq, R.LATENT:] = latent.to_numpy().view(np.uint16), kpe.to_numpy().view(np.uint16)[:, 0]
    np.testing.assert_array_equal(cache.to_numpy().view(np.uint16), want)


@pytest.mark.parametrize("q_lora", [None, 96])
def test_layer_against_the_textbook_oracle(q_lora):
    """Chunks of 12 and 3 tokens, then 4 single tokens through the latent cache, against the NON-absorbed oracle at the model bar."""
    from pygpukit_amd.llm.layers import MLAttention

    w, (_, heads, nope, v) = R.make_weights(5, q_lora), R.LAYER.values()
    layer = MLAttention(num_heads=heads, qk_nope_head_dim=nope, v_head_dim=v, softmax_scale=R.LAYER_SCALE, max_position_embeddings=64,
                        **{k: _dev(a) for k, a in w.items()})
    layer.init_fixed_cache(40, "bfloat16")
    ref, start = R.Layer(w, heads, nope, v, R.LAYER_SCALE), 0
    for x in R.layer_inputs():
        e = rel_err(_host(layer.forward_fixed_cache(_dev(x), start), "bf16"), ref(x))
        print(f"q_lora {q_lora}, rows {start}..{start + x.shape[0] - 1}: rel_err {e:.3e}")
        assert e <= 1e-2
        start += x.shape[0]
