"""Batched MLA decode over a paged latent cache on the GPU against the float64 oracle tests/mla_paged_ref.py.  Bar: the project's MLA
bar, rel_err <= 1e-2; the unavoidable roundings alone stay under 5e-3 at these shapes (test_mla_paged_cpu.py)."""

import numpy as np
import pytest

from tests import attn_stair_ref as S
from tests import mla_paged_ref as P
from tests import mla_ref as R
from tests.conftest import rel_err
from tests.test_mla_gpu import _dev, _host, _words          # uint16 words <-> device arrays

pytestmark = pytest.mark.gpu

LONG = {"bf16": "bfloat16", "f16": "float16"}


def _i32(x):
    from pygpukit_amd.core import from_numpy

    return from_numpy(np.ascontiguousarray(x, np.int32))


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("bound", P.BOUNDS)
@pytest.mark.parametrize("block_size", P.BLOCK_SIZES)
@pytest.mark.parametrize("q_len,heads", P.OP_SHAPES)
def test_op_against_the_oracle(q_len, heads, block_size, bound, dtype):
    """Six sequences of very different lengths, one idle, in one launch; NaN in `out` beforehand and in everything the kernel must not read."""
    from pygpukit_amd.ops.nn import sdpa_mla_paged, sdpa_mla_paged_plan

    ctxs = P.contexts(q_len, bound)
    assert (sdpa_mla_paged_plan(heads, q_len, len(ctxs), bound, LONG[dtype])[1][1] > 1) == (bound == 640)
    q, rows, pages, tables = P.case(q_len, heads, block_size, ctxs, dtype)
    out = _words(np.full(q.shape[:3] + (R.LATENT,), pages[0, 0, 0], np.uint16), dtype)
    sdpa_mla_paged(_dev(q, dtype), _words(pages, dtype), _i32(tables), _i32(ctxs), out, bound, R.SCALE)
    got = _host(out, dtype)
    assert np.isfinite(got).all() and not got[0].any()
    e = rel_err(got, P.op(q, rows, ctxs, R.SCALE))
    print(f"rel_err {e:.3e}")
    assert e <= 1e-2


def test_lengths_are_read_on_the_device():
    """One set of launch arguments; only the int32 lengths on the device change between the calls (40 -> 41 -> 600 under the bound 640)."""
    from pygpukit_amd.ops.nn import sdpa_mla_paged

    full, steps = (600, 600), ((40, 600), (41, 40), (600, 41))
    q, rows, pages, tables = P.case(1, 20, 48, full, "bf16")
    args = _dev(q), _words(pages, "bf16"), _i32(tables), _i32(full), _words(np.zeros(q.shape[:3] + (R.LATENT,), np.uint16), "bf16")
    for ctxs in steps:
        args[3].copy_from_numpy(np.array(ctxs, np.int32))
        sdpa_mla_paged(*args, 640, R.SCALE)
        e = rel_err(_host(args[4], "bf16"), P.op(q, [r[:c] for r, c in zip(rows, ctxs)], ctxs, R.SCALE))
        print(f"contexts {ctxs}: rel_err {e:.3e}")
        assert e <= 1e-2


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("table", ["f32", "same"])
@pytest.mark.parametrize("block_size", [16, 48])
def test_writer_bits(block_size, table, dtype):
    """Seven tokens at shuffled positions into shuffled slots, one slot negative: a written slot holds mla_cache_write's row for that
    position, bit for bit, and every other byte of the pages is untouched."""
    from pygpukit_amd.core import from_numpy
    from pygpukit_amd.llm.layers.rope import precompute_freqs_cis
    from pygpukit_amd.ops.nn import mla_cache_write, mla_reshape_and_cache

    rng, n, blocks, max_pos = np.random.default_rng(block_size), 7, 3, 40
    kv_a, gamma = S.round_to(rng.standard_normal((n, R.WIDTH)) * 3.0, dtype), S.round_to(1.0 + 0.2 * rng.standard_normal(R.LATENT), dtype)
    up = from_numpy if table == "f32" else (lambda a: _dev(a, dtype))
    cos, sin = (up(np.ascontiguousarray(t, np.float32)) for t in precompute_freqs_cis(R.ROPE, max_pos))
    pos, slots = rng.permutation(max_pos)[:n], rng.permutation(blocks * block_size)[:n]
    slots[3] = -1
    pages, flat = (_words(np.full(s, 0xA5A5, np.uint16), dtype) for s in ((blocks, block_size, R.WIDTH), (max_pos, R.WIDTH)))
    mla_reshape_and_cache(_dev(kv_a, dtype), _dev(gamma, dtype), cos, sin, _i32(pos), pages, _i32(slots), 1e-6)
    for t in range(n):
        mla_cache_write(_dev(kv_a[t:t + 1], dtype), _dev(gamma, dtype), cos, sin, flat, int(pos[t]), 1e-6)
    want, keep = np.full((blocks * block_size, R.WIDTH), 0xA5A5, np.uint16), slots >= 0
    want[slots[keep]] = flat.to_numpy().view(np.uint16)[pos[keep]]
    np.testing.assert_array_equal(pages.to_numpy().view(np.uint16).reshape(want.shape), want)


@pytest.mark.parametrize("q_lora", [None, 96])
def test_layer_against_the_textbook_oracle_and_the_fixed_cache(q_lora):
    """Three sequences prefilled to 5, 17 and 30 rows through mla_reshape_and_cache, then three batched decode steps: every row against
    the NON-absorbed oracle of its sequence and against forward_fixed_cache run for that sequence alone."""
    from pygpukit_amd.llm.layers import MLAttention
    from pygpukit_amd.ops.nn import allocate_mla_cache, mla_reshape_and_cache

    w, (hidden, heads, nope, v), lens, bs = R.make_weights(5, q_lora), R.LAYER.values(), [5, 17, 30], 16
    make = lambda: MLAttention(num_heads=heads, qk_nope_head_dim=nope, v_head_dim=v, softmax_scale=R.LAYER_SCALE,  # noqa: E731
                               max_position_embeddings=64, **{k: _dev(a) for k, a in w.items()})
    layer, fixed, refs = make(), [make() for _ in lens], [R.Layer(w, heads, nope, v, R.LAYER_SCALE) for _ in lens]
    rng = np.random.default_rng(9)
    tables = rng.permutation(12).reshape(4, 3).T.astype(np.int32)          # [3 sequences, 4 pages], interleaved
    cache = allocate_mla_cache(12, bs, "bfloat16")
    slot = lambda b, p: tables[b, p // bs] * bs + p % bs  # noqa: E731
    for b, n in enumerate(lens):
        x = S.round_to(rng.standard_normal((n, hidden)), "bf16").astype(np.float64)
        fixed[b].init_fixed_cache(40)
        fixed[b].forward_fixed_cache(_dev(x), 0), refs[b](x)
        mla_reshape_and_cache(layer.kv_a_proj_with_mqa(_dev(x)), layer.kv_a_layernorm, layer._cos, layer._sin, _i32(np.arange(n)), cache,
                              _i32([slot(b, p) for p in range(n)]), 1e-6)
    for _ in range(3):
        x = S.round_to(rng.standard_normal((len(lens), hidden)), "bf16").astype(np.float64)
        got = _host(layer.forward_paged(_dev(x), _i32(lens), _i32([slot(b, p) for b, p in enumerate(lens)]), _i32(tables),
                                        _i32([n + 1 for n in lens]), cache, 64), "bf16")
        for b, n in enumerate(lens):
            e_ref = rel_err(got[b], refs[b](x[b:b + 1])[0])
            e_fix = rel_err(got[b], _host(fixed[b].forward_fixed_cache(_dev(x[b:b + 1]), n), "bf16")[0])
            print(f"q_lora {q_lora}, sequence {b} at {n}: rel_err {e_ref:.3e} (oracle), {e_fix:.3e} (fixed cache)")
            assert e_ref <= 1e-2 and e_fix <= 1e-2
        lens = [n + 1 for n in lens]
