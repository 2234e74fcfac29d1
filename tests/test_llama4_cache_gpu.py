"""GPU tests of the Llama-4 KV-cache decode: llama4_qk_norm_cache_write, sdpa_irope_fixed_cache, their _ptr forms and the
model's init_fixed_cache / prefill_fixed_cache / decode_step / capture_decode / decode_step_graph / generate(use_cache).

Bars.  Attention and logits: rel_err <= 1e-2 against the NumPy restatements (tests/llama4_ref.py,
tests/llama4_cache_ref.py) on bf16-rounded inputs - the bar of the existing Llama-4 GPU tests; the decode kernel keeps
Q * t in fp32, so it rounds less than the prefill kernel that meets the same bar.  Bit-identity where the new path runs
the same arithmetic on the same values: the prep kernel against l2norm + kv_cache_prefill_gqa, the _ptr and graph forms
against the host forms, prefill_fixed_cache against forward.  No test hands the device a position beyond the cache."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from oracle import cpu_ref as O
from tests import llama4_cache_ref as C
from tests import llama4_ref as R
from tests.conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

BAR = 1e-2
MAX_SEQ = 1024          # 4 KV splits
ATTN_SCALE, FLOOR_SCALE = 0.5, 16.0          # the temperature steps every 16 positions
NAN_BITS = {"bf16": 0x7FC0, "f16": 0x7E00}


def _bits(x, dtype) -> np.ndarray:
    """float32 values -> the 16-bit words of `dtype`."""
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


def _i32(v):
    from pygpukit_amd.core import from_numpy

    return from_numpy(np.array([v], np.int32))


# ---- sdpa_irope_fixed_cache --------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _qkv(hq, hkv, d, dtype, max_seq=MAX_SEQ):
    """Seeded Q [Hq,1,D] and full caches [Hkv,max_seq,D] as 16-bit words (read-only, shared by the cases)."""
    rng = np.random.default_rng(7000 + 100 * hq + 10 * hkv + d)
    q, k, v = (_bits(rng.standard_normal(s).astype(np.float32), dtype) for s in ((hq, 1, d), (hkv, max_seq, d), (hkv, max_seq, d)))
    for a in (q, k, v):
        a.setflags(write=False)
    return q, k, v


@functools.lru_cache(maxsize=None)
def _want(hq, hkv, d, dtype, pos, attn_scale=ATTN_SCALE, max_seq=MAX_SEQ):
    q, k, v = (_values(a, dtype) for a in _qkv(hq, hkv, d, dtype, max_seq))
    want = R.sdpa_irope(q, k[:, :pos + 1], v[:, :pos + 1], np.array([pos]), attn_scale, FLOOR_SCALE, pos)
    want.setflags(write=False)
    return want


def _caches(hq, hkv, d, dtype, pos, max_seq=MAX_SEQ):
    """Device Q and caches whose rows beyond `pos` hold NaN: a kernel that reads one row too many returns NaN."""
    q, k, v = _qkv(hq, hkv, d, dtype, max_seq)
    k, v = k.copy(), v.copy()
    k[:, pos + 1:] = NAN_BITS[dtype]
    v[:, pos + 1:] = NAN_BITS[dtype]
    return _dev_bits(q, dtype), _dev_bits(k, dtype), _dev_bits(v, dtype)


def _nan_out(shape, dtype):
    return _dev_bits(np.full(shape, NAN_BITS[dtype], np.uint16), dtype)


def _attend(hq, hkv, d, dtype, pos, attn_scale=ATTN_SCALE, max_seq=MAX_SEQ):
    from pygpukit_amd.ops.nn import sdpa_irope_fixed_cache

    qd, kd, vd = _caches(hq, hkv, d, dtype, pos, max_seq)
    out = _nan_out((hq, 1, d), dtype)           # NaN everywhere: every element must be written
    sdpa_irope_fixed_cache(qd, kd, vd, out, pos, attn_scale, FLOOR_SCALE)
    words = _host_bits(out)
    assert np.isfinite(_values(words, dtype)).all()
    return words


@pytest.mark.parametrize("pos", [0, 69, 255, 256, 1023])      # three empty splits .. first row of the second chunk .. full cache
def test_fixed_cache_attention_matches_the_restatement_at_every_split_boundary(pos):
    err = rel_err(_values(_attend(4, 2, 128, "bf16", pos), "bf16"), _want(4, 2, 128, "bf16", pos))
    print(f"sdpa_irope_fixed_cache (4,2) D 128 pos {pos}: rel_err {err:.3e}")
    assert err <= BAR


@pytest.mark.parametrize("hq,hkv", [(2, 2), (4, 2), (8, 2), (5, 1), (40, 8)])      # Hq / Hkv = 1, 2, 4, 5, 5
def test_fixed_cache_attention_every_head_grouping(hq, hkv):
    err = rel_err(_values(_attend(hq, hkv, 128, "bf16", 300), "bf16"), _want(hq, hkv, 128, "bf16", 300))
    print(f"sdpa_irope_fixed_cache ({hq},{hkv}) D 128 pos 300: rel_err {err:.3e}")
    assert err <= BAR


@pytest.mark.parametrize("pos", [300, 8191])      # 10 of the 32 splits hold rows; the full cache
def test_fixed_cache_attention_five_heads_per_workgroup(pos):
    """Hq / Hkv = 5 takes the five-heads-per-workgroup kernel only where that grid has 256 workgroups: 40 / 8 heads need
    32 KV splits, a cache of 8192 rows (at MAX_SEQ the cases above run one head per workgroup)."""
    err = rel_err(_values(_attend(40, 8, 128, "bf16", pos, max_seq=8192), "bf16"), _want(40, 8, 128, "bf16", pos, max_seq=8192))
    print(f"sdpa_irope_fixed_cache (40,8) D 128 cache 8192 pos {pos}: rel_err {err:.3e}")
    assert err <= BAR


def test_fixed_cache_attention_head_dim_64_float16():
    err = rel_err(_values(_attend(4, 2, 64, "f16", 300), "f16"), _want(4, 2, 64, "f16", 300))
    print(f"sdpa_irope_fixed_cache (4,2) D 64 f16 pos 300: rel_err {err:.3e}")
    assert err <= BAR


def test_fixed_cache_attention_applies_the_temperature():
    with_t = _values(_attend(4, 2, 128, "bf16", 300), "bf16")
    without = _values(_attend(4, 2, 128, "bf16", 300, attn_scale=0.0), "bf16")
    diff = rel_err(with_t, without)
    print(f"attn_scale 0.5 against attn_scale 0 at pos 300: rel_err {diff:.3e}")
    assert diff > BAR
    assert rel_err(without, _want(4, 2, 128, "bf16", 300, 0.0)) <= BAR


def test_fixed_cache_attention_ptr_form_and_graph_replay_are_bit_identical():
    import pygpukit_amd as pk
    from pygpukit_amd.ops.nn import sdpa_irope_fixed_cache_ptr

    host = {pos: _attend(4, 2, 128, "bf16", pos) for pos in (69, 256)}
    for pos in (69, 256):
        qd, kd, vd = _caches(4, 2, 128, "bf16", pos)
        out = _nan_out((4, 1, 128), "bf16")
        sdpa_irope_fixed_cache_ptr(qd, kd, vd, out, _i32(pos), ATTN_SCALE, FLOOR_SCALE)
        np.testing.assert_array_equal(_host_bits(out), host[pos])
    # captured once with 69 in the device buffer, replayed, then replayed after the buffer is rewritten to 256; the caches
    # hold rows 0 .. 256 (NaN beyond), which both positions may read
    qd, kd, vd = _caches(4, 2, 128, "bf16", 256)
    out, pbuf = _nan_out((4, 1, 128), "bf16"), _i32(69)
    graph = pk.CudaGraph()
    graph.begin_capture()
    sdpa_irope_fixed_cache_ptr(qd, kd, vd, out, pbuf, ATTN_SCALE, FLOOR_SCALE)
    graph.end_capture()
    graph.replay()
    graph.synchronize()
    np.testing.assert_array_equal(_host_bits(out), host[69])
    pbuf.copy_from_numpy(np.array([256], np.int32))
    graph.replay()
    graph.synchronize()
    np.testing.assert_array_equal(_host_bits(out), host[256])


# ---- llama4_qk_norm_cache_write ----------------------------------------------------------------------------------------

PREP_MAX_SEQ = 160
SENTINEL = 0xABCD
EPS = 1e-5


def _prep_inputs(S, hq, hkv, d, dtype):
    rng = np.random.default_rng(S + 10 * hq + d)
    return tuple(_bits(rng.standard_normal((S, h * d)).astype(np.float32) * np.float32(3.0), dtype) for h in (hq, hkv, hkv))


def _sentinel_caches(hkv, d, dtype):
    return tuple(_dev_bits(np.full((hkv, PREP_MAX_SEQ, d), SENTINEL, np.uint16), dtype) for _ in range(2))


def _composition(q, k, v, S, pos, hq, hkv, d, dtype, qk_norm=True):
    """The ops the prep kernel replaces: l2norm on the q and k head rows, kv_cache_prefill_gqa with num_heads = Hkv."""
    from pygpukit_amd.ops.basic import kv_cache_prefill_gqa
    from pygpukit_amd.ops.nn import l2norm

    qd, kd, vd = (_dev_bits(a, dtype) for a in (q, k, v))
    kc, vc = _sentinel_caches(hkv, d, dtype)
    if qk_norm:
        qf, kf = qd.view((S * hq, d)), kd.view((S * hkv, d))
        l2norm(qf, EPS, out=qf)
        l2norm(kf, EPS, out=kf)
    kv_cache_prefill_gqa(kd.view((S, hkv, d)), kc, hkv, pos)
    kv_cache_prefill_gqa(vd.view((S, hkv, d)), vc, hkv, pos)
    return _host_bits(qd), _host_bits(kc), _host_bits(vc)


def _prep(q, k, v, pos, hq, hkv, d, dtype, qk_norm=True, ptr=False):
    from pygpukit_amd.ops.nn import llama4_qk_norm_cache_write, llama4_qk_norm_cache_write_ptr

    qd, kd, vd = (_dev_bits(a, dtype) for a in (q, k, v))
    kc, vc = _sentinel_caches(hkv, d, dtype)
    kw = dict(num_heads=hq, num_kv_heads=hkv, head_dim=d, eps=EPS, qk_norm=qk_norm)
    if ptr:
        llama4_qk_norm_cache_write_ptr(qd, kd, vd, kc, vc, _i32(pos), **kw)
    else:
        llama4_qk_norm_cache_write(qd, kd, vd, kc, vc, pos, **kw)
    np.testing.assert_array_equal(_host_bits(kd), k)          # k and v themselves are inputs only
    np.testing.assert_array_equal(_host_bits(vd), v)
    return _host_bits(qd), _host_bits(kc), _host_bits(vc)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("hq,hkv,d", [(4, 2, 64), (5, 1, 128)])
@pytest.mark.parametrize("S,pos", [(1, 0), (1, PREP_MAX_SEQ - 1), (5, 7), (130, 0)])
def test_prep_kernel_is_bit_identical_to_the_ops_it_replaces(S, pos, hq, hkv, d, dtype):
    q, k, v = _prep_inputs(S, hq, hkv, d, dtype)
    want_q, want_kc, want_vc = _composition(q, k, v, S, pos, hq, hkv, d, dtype)
    got_q, got_kc, got_vc = _prep(q, k, v, pos, hq, hkv, d, dtype)
    np.testing.assert_array_equal(got_q, want_q)              # Q normalised in place
    np.testing.assert_array_equal(got_kc, want_kc)            # written rows and, with them, every untouched row
    np.testing.assert_array_equal(got_vc, want_vc)
    written = np.zeros(PREP_MAX_SEQ, bool)
    written[pos:pos + S] = True
    assert (got_kc[:, ~written] == SENTINEL).all() and (got_vc[:, ~written] == SENTINEL).all()
    assert (got_q != q).any() and (got_kc[:, written] != SENTINEL).any()
    # the _ptr form gives the same bits
    for got, want in zip(_prep(q, k, v, pos, hq, hkv, d, dtype, ptr=True), (got_q, got_kc, got_vc)):
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("ptr", [False, True])
def test_prep_kernel_without_qk_norm_copies(ptr):
    S, pos, hq, hkv, d = 5, 7, 5, 1, 128
    q, k, v = _prep_inputs(S, hq, hkv, d, "bf16")
    got_q, got_kc, got_vc = _prep(q, k, v, pos, hq, hkv, d, "bf16", qk_norm=False, ptr=ptr)
    np.testing.assert_array_equal(got_q, q)
    np.testing.assert_array_equal(got_kc[:, pos:pos + S], k.reshape(S, hkv, d).transpose(1, 0, 2))
    np.testing.assert_array_equal(got_vc[:, pos:pos + S], v.reshape(S, hkv, d).transpose(1, 0, 2))
    want = _composition(q, k, v, S, pos, hq, hkv, d, "bf16", qk_norm=False)
    for got, w in zip((got_q, got_kc, got_vc), want):
        np.testing.assert_array_equal(got, w)


# ---- model -------------------------------------------------------------------------------------------------------------

PROMPT, STEPS = 12, 24


def _build_model():
    from pygpukit_amd.core import from_numpy
    from pygpukit_amd.llm.models.llama4 import Llama4Attention, Llama4Block, Llama4Config, Llama4MLP, Llama4Model

    g = load_golden("g7_llama4.npz")
    w = R.make_llama4_weights(R.TINY_CFG, int(g["model_seed"]))
    cfg = Llama4Config(**R.TINY_CFG)
    W = lambda a: from_numpy(O.f32_to_bf16_bits(a))          # noqa: E731  (weights are bf16-representable: exact)
    blocks = [Llama4Block(Llama4Attention(W(lw["q"]), W(lw["k"]), W(lw["v"]), W(lw["o"]), cfg),
                          Llama4MLP(W(lw["gate"]), W(lw["up"]), W(lw["down"])), W(lw["input_norm"]), W(lw["post_norm"]), cfg.rms_norm_eps)
              for lw in w["layers"]]
    return Llama4Model(cfg, W(w["embed"]), blocks, W(w["norm"]), W(w["lm_head"])), w, g


@functools.lru_cache(maxsize=None)
def _tiny_model():
    return _build_model()


@functools.lru_cache(maxsize=None)
def _teacher():
    """(the g7 prompt + 24 greedy tokens of the restatement, the cached restatement's logits for those 36 rows)."""
    _, w, g = _tiny_model()
    ids, _ = R.generate(R.TINY_CFG, w, g["model_prompt"], STEPS)
    ids = ids[:PROMPT + STEPS]
    want = C.teacher_forced(R.TINY_CFG, w, ids, PROMPT)
    ids.setflags(write=False)
    want.setflags(write=False)
    return ids, want


def _logits(a) -> np.ndarray:
    return O.bf16_bits_to_f32(a.to_numpy())


def test_prefill_fixed_cache_is_bit_identical_to_forward():
    model, _, g = _tiny_model()
    model.init_fixed_cache(PROMPT + STEPS)
    got = model.prefill_fixed_cache(g["model_prompt"])
    assert got.shape == (PROMPT, 100)
    np.testing.assert_array_equal(got.to_numpy(), model.forward(g["model_prompt"]).to_numpy())
    assert rel_err(_logits(got), g["model_logits"]) <= BAR


def test_prefill_fixed_cache_in_two_chunks():
    model, _, g = _tiny_model()
    model.init_fixed_cache(PROMPT + STEPS)
    first = model.prefill_fixed_cache(g["model_prompt"][:5])
    second = model.prefill_fixed_cache(g["model_prompt"][5:], start_pos=5)
    got = np.concatenate([_logits(first), _logits(second)])
    assert np.isfinite(got).all()
    err = rel_err(got, g["model_logits"])
    print(f"prefill 5 + 7: rel_err {err:.3e}")
    assert err <= BAR


def test_teacher_forced_decode_steps_match_the_restatement_and_the_graph_matches_eager():
    """24 one-token steps on the restatement's own tokens (positions 12 .. 35).  Measured on an MI355X: worst step
    rel_err 9.0e-3 (the tiny model's prefill logits sit at 6.4e-3 under the same bar)."""
    model, _, g = _tiny_model()
    ids, want = _teacher()
    model.init_fixed_cache(PROMPT + STEPS)
    model.prefill_fixed_cache(ids[:PROMPT])
    model.capture_decode()
    worst = 0.0
    for pos in range(PROMPT, PROMPT + STEPS):
        eager = model.decode_step(int(ids[pos]), pos)
        assert eager.shape == (1, 100)
        eager = eager.to_numpy()
        got = O.bf16_bits_to_f32(eager)
        assert np.isfinite(got).all()
        err = rel_err(got, want[pos:pos + 1])
        worst = max(worst, err)
        assert err <= BAR, (pos, err)
        replayed = model.decode_step_graph(int(ids[pos]), pos).to_numpy()       # rewrites row `pos` with the same values
        np.testing.assert_array_equal(replayed, eager, err_msg=f"position {pos}")
    print(f"24 teacher-forced decode steps: worst rel_err {worst:.3e}")
    t = R.irope_temperature(np.arange(PROMPT, PROMPT + STEPS), R.TINY_CFG["attn_scale"], R.TINY_CFG["floor_scale"])
    assert len(set(t.tolist())) == 7          # the temperature steps at 15, 19, ..., 35


@pytest.mark.parametrize("use_graph", [False, True])
def test_generate_with_cache_returns_the_recorded_tokens(use_graph):
    from pygpukit_amd.llm.models.llama4 import generate

    model, _, g = _tiny_model()
    ids = generate(model, g["model_prompt"], max_new_tokens=6, eos_token_id=-1, use_cache=True, use_graph=use_graph)
    assert ids.dtype == np.int64
    np.testing.assert_array_equal(ids[:PROMPT], g["model_prompt"])
    np.testing.assert_array_equal(ids[PROMPT:], g["model_tokens"])
    # eos stops the cached loop after the token is appended, as in the uncached loop
    eos = int(g["model_tokens"][1])
    stop = generate(model, g["model_prompt"], max_new_tokens=6, eos_token_id=[eos], use_cache=True, use_graph=use_graph)
    np.testing.assert_array_equal(stop[PROMPT:], g["model_tokens"][:list(g["model_tokens"]).index(eos) + 1])


def test_generate_allocates_a_cache_when_the_model_has_none():
    from pygpukit_amd.llm.models.llama4 import generate

    model, _, g = _build_model()
    assert model.max_cache_len == 0
    ids = generate(model, g["model_prompt"], max_new_tokens=6, eos_token_id=-1, use_cache=True)
    np.testing.assert_array_equal(ids[PROMPT:], g["model_tokens"])
    assert model.max_cache_len == PROMPT + 6


# ---- refused cases -----------------------------------------------------------------------------------------------------

def test_refused_cases():
    from pygpukit_amd import _hip
    from pygpukit_amd.core import from_numpy
    from pygpukit_amd.ops.nn import (llama4_qk_norm_cache_write, llama4_qk_norm_cache_write_ptr, sdpa_irope_fixed_cache,
                                     sdpa_irope_fixed_cache_ptr)

    bf = lambda *s: from_numpy(np.zeros(s, np.uint16))       # noqa: E731
    f32 = lambda *s: from_numpy(np.zeros(s, np.float32))     # noqa: E731
    kw = dict(num_heads=4, num_kv_heads=2, head_dim=128, eps=1e-5)
    # attention
    with pytest.raises(ValueError, match="head_dim"):
        sdpa_irope_fixed_cache(bf(4, 1, 96), bf(2, 64, 96), bf(2, 64, 96), bf(4, 1, 96), 3)
    with pytest.raises(ValueError):
        sdpa_irope_fixed_cache(f32(4, 1, 128), f32(2, 64, 128), f32(2, 64, 128), f32(4, 1, 128), 3)          # float32
    with pytest.raises(ValueError, match="n_heads"):
        sdpa_irope_fixed_cache(bf(3, 1, 128), bf(2, 64, 128), bf(2, 64, 128), bf(3, 1, 128), 3)
    with pytest.raises(ValueError, match="outside cache"):
        sdpa_irope_fixed_cache(bf(4, 1, 128), bf(2, 64, 128), bf(2, 64, 128), bf(4, 1, 128), 64)             # position >= max_seq
    with pytest.raises(ValueError, match="outside cache"):
        sdpa_irope_fixed_cache(bf(4, 1, 128), bf(2, 64, 128), bf(2, 64, 128), bf(4, 1, 128), -1)
    with pytest.raises(ValueError, match="caches"):
        sdpa_irope_fixed_cache(bf(4, 1, 128), bf(2, 64, 128), bf(2, 32, 128), bf(4, 1, 128), 3)              # K / V differ
    with pytest.raises(ValueError, match="q_len"):
        sdpa_irope_fixed_cache(bf(4, 2, 128), bf(2, 64, 128), bf(2, 64, 128), bf(4, 2, 128), 3)
    with pytest.raises(ValueError, match="int32"):
        sdpa_irope_fixed_cache_ptr(bf(4, 1, 128), bf(2, 64, 128), bf(2, 64, 128), bf(4, 1, 128), from_numpy(np.zeros(1, np.int64)))
    # prep kernel
    with pytest.raises(ValueError, match="head_dim"):
        llama4_qk_norm_cache_write(bf(1, 384), bf(1, 192), bf(1, 192), bf(2, 64, 96), bf(2, 64, 96), 0, **{**kw, "head_dim": 96})
    with pytest.raises(ValueError):
        llama4_qk_norm_cache_write(f32(1, 512), f32(1, 256), f32(1, 256), f32(2, 64, 128), f32(2, 64, 128), 0, **kw)
    with pytest.raises(ValueError, match="n_heads"):
        llama4_qk_norm_cache_write(bf(1, 384), bf(1, 256), bf(1, 256), bf(2, 64, 128), bf(2, 64, 128), 0, **{**kw, "num_heads": 3})
    with pytest.raises(ValueError, match="outside cache"):
        llama4_qk_norm_cache_write(bf(1, 512), bf(1, 256), bf(1, 256), bf(2, 64, 128), bf(2, 64, 128), 64, **kw)
    with pytest.raises(ValueError, match="outside cache"):
        llama4_qk_norm_cache_write(bf(5, 512), bf(5, 256), bf(5, 256), bf(2, 64, 128), bf(2, 64, 128), 60, **kw)   # last row at 64
    with pytest.raises(ValueError, match="caches"):
        llama4_qk_norm_cache_write(bf(1, 512), bf(1, 256), bf(1, 256), bf(2, 64, 128), bf(4, 64, 128), 0, **kw)
    with pytest.raises(ValueError, match="k "):
        llama4_qk_norm_cache_write(bf(2, 512), bf(1, 256), bf(2, 256), bf(2, 64, 128), bf(2, 64, 128), 0, **kw)
    with pytest.raises(ValueError, match="int32"):
        llama4_qk_norm_cache_write_ptr(bf(1, 512), bf(1, 256), bf(1, 256), bf(2, 64, 128), bf(2, 64, 128), f32(1), **kw)
    # the native entries refuse the same on their own, with a message
    q, kc, o, ws = bf(4, 1, 128), bf(2, 64, 128), bf(4, 1, 128), f32(4 * 130)
    BF16, F32 = q.dtype.code, ws.dtype.code

    def attend(hq=4, hkv=2, d=128, pos=3, dt=BF16):
        _hip.call("pgk_sdpa_irope_fixed_cache", q._p, kc._p, kc._p, o._p, hq, hkv, 64, d, 0.1, 8192.0, pos, None, ws._p, dt, None)

    def prep(hq=4, hkv=2, d=128, pos=3, seq=1, dt=BF16):
        _hip.call("pgk_llama4_qk_norm_cache_write", q._p, kc._p, kc._p, kc._p, kc._p, seq, hq, hkv, 64, d, 1e-5, 1, pos, None, dt, None)

    for fn, name in ((attend, "pgk_sdpa_irope_fixed_cache"), (prep, "pgk_llama4_qk_norm_cache_write")):
        with pytest.raises(RuntimeError, match=name + ": float16 / bfloat16 only"):
            fn(dt=F32)
        with pytest.raises(RuntimeError, match=name + ": head_dim must be 64 or 128"):
            fn(d=96)
        with pytest.raises(RuntimeError, match=name + ": n_heads mismatch"):
            fn(hq=3)
        with pytest.raises(RuntimeError, match="outside cache"):
            fn(pos=64)
    with pytest.raises(RuntimeError, match="outside cache"):
        prep(pos=63, seq=2)
    attend()          # and accept the valid call


def test_model_refusals():
    model, _, g = _build_model()
    with pytest.raises(RuntimeError, match="init_fixed_cache"):
        model.decode_step(1, 0)
    with pytest.raises(RuntimeError, match="init_fixed_cache"):
        model.prefill_fixed_cache(g["model_prompt"])
    with pytest.raises(RuntimeError, match="init_fixed_cache"):
        model.capture_decode()
    model.init_fixed_cache(8)
    with pytest.raises(RuntimeError, match="capture_decode"):
        model.decode_step_graph(1, 0)
    with pytest.raises(ValueError, match="outside the cache"):
        model.prefill_fixed_cache(g["model_prompt"])                 # 12 rows into a cache of 8
    with pytest.raises(ValueError, match="outside the cache"):
        model.prefill_fixed_cache(g["model_prompt"][:4], start_pos=5)
    with pytest.raises(ValueError, match="outside the cache"):
        model.decode_step(1, 8)
    with pytest.raises(ValueError, match="token id"):
        model.decode_step(100, 0)
    model.capture_decode()
    model.decode_step_graph(1, 0)
    model.init_fixed_cache(8)                                        # new caches: the captured graph addresses the old ones
    with pytest.raises(RuntimeError, match="capture_decode"):
        model.decode_step_graph(1, 0)
