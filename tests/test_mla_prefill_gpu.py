"""sdpa_mla_prefill and MLAttention.forward_prefill on the GPU against the float64 oracles tests/mla_prefill_ref.py and mla_ref.Layer.
Bar: rel_err <= 1e-2, what every 16-bit attention parity test here holds; the kernel's unavoidable roundings alone stay under a third of
it (test_mla_prefill_cpu.py).  The kernel's tiles are the issue's (128 query rows, 32 per wave, 64 keys), so are the shapes."""

import numpy as np
import pytest

from tests import attn_stair_ref as S
from tests import mla_prefill_ref as P
from tests import mla_ref as R
from tests.conftest import rel_err
from tests.test_mla_gpu import NAN, _dev, _host, _words

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", ["bf16", "f16"])


def _run(q_nope, q_pe, kv, kpe, dtype, scale):
    """NaN words in the cache rows >= T, in the latent columns of every row (the kernel reads neither) and in the whole of out."""
    from pygpukit_amd.ops.nn import sdpa_mla_prefill

    (s_len, heads, _), t_len = q_nope.shape, kv.shape[0]
    cache = np.full((t_len + 3, R.WIDTH), NAN[dtype], np.uint16)
    cache[:t_len, R.LATENT:] = S.to_words(kpe, dtype)
    out = _words(np.full((s_len, heads, P.V), NAN[dtype], np.uint16), dtype)
    sdpa_mla_prefill(_dev(q_nope, dtype), _dev(q_pe, dtype), _dev(kv, dtype), _words(cache, dtype), out, t_len, scale)
    return _host(out, dtype)


@DTYPES
@pytest.mark.parametrize("shape", P.SHAPES)
def test_against_the_oracle(shape, dtype):
    got = _run(*P.case(*shape, dtype), dtype, R.SCALE)
    assert np.isfinite(got).all()
    e = rel_err(got, P.exact(*shape, dtype))
    print(f"{shape} {dtype}: rel_err {e:.3e}")
    assert e <= 1e-2


@DTYPES
@pytest.mark.parametrize("gap", [64, 128])
@pytest.mark.parametrize("shape", [(5, 70, 3), (130, 321, 2)])
def test_mask_on_a_staircase(shape, gap, dtype):
    """test_mla_gpu's staircase on this kernel: columns 0 / 1 of k_nope hold j >> 4 and j & 15 and every query 16 g and g there,
    g = gap / scale, so the score of key j is gap * j plus a few units of noise and an off-by-one of the mask either way moves the
    output to another row.  gap 128: every other exp2 is 0 in fp32, the output IS the last visible row's v, bit for bit."""
    scale, (s_len, t_len, _) = 0.125, shape
    q_nope, q_pe, kv, kpe = (np.array(a) for a in P.case(*shape, dtype))
    j = np.arange(t_len)[:, None]
    kv[..., 0], kv[..., 1], q_nope[..., 0], q_nope[..., 1] = j >> 4, j & 15, 16 * gap / scale, gap / scale
    got, want = _run(q_nope, q_pe, kv, kpe, dtype, scale), kv[t_len - s_len:, :, P.NOPE:]
    if gap == 128:
        np.testing.assert_array_equal(got, want)
    else:
        assert np.isfinite(got).all() and rel_err(got, P.op(q_nope, q_pe, kv, kpe, scale)) <= 1e-2 and rel_err(got, want) <= 1e-2


@pytest.mark.parametrize("q_lora", [None, 96])
def test_layer_against_the_textbook_oracle(q_lora):
    """Chunks of 70 and 3 tokens through forward_prefill, then three single tokens through forward_fixed_cache on the same cache."""
    from pygpukit_amd.llm.layers import MLAttention

    w, (hidden, heads, nope, v), start = P.make_weights(5, q_lora), P.LAYER.values(), 0
    layer = MLAttention(num_heads=heads, qk_nope_head_dim=nope, v_head_dim=v, softmax_scale=R.SCALE, max_position_embeddings=128,
                        **{k: _dev(a) for k, a in w.items()})
    layer.init_fixed_cache(sum(P.LAYER_CHUNKS) + 4, "bfloat16")
    ref, rng = R.Layer(w, heads, nope, v, R.SCALE), np.random.default_rng(77)
    for n in P.LAYER_CHUNKS:
        x = S.round_to(rng.standard_normal((n, hidden)), "bf16").astype(np.float64)
        forward = layer.forward_prefill if n > 1 else layer.forward_fixed_cache
        e = rel_err(_host(forward(_dev(x), start), "bf16"), ref(x))
        print(f"q_lora {q_lora}, rows {start}..{start + n - 1}: rel_err {e:.3e}")
        assert e <= 1e-2
        start += n
