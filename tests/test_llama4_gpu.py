"""GPU tests of the Llama-4 ops and model against the NumPy restatement (tests/llama4_ref.py) and the reference's recorded
results (tests/golden/g7_llama4.npz).

Bars: attention, l2norm and the model's logits must be within rel_err 1e-2 of the restatement on bf16-rounded inputs -
the project's bf16 bar, which sdpa_causal meets with the same kernel structure; the only new arithmetic in sdpa_irope
is one fp32 factor inside the existing rounding of the Q fragment.  float32 l2norm: 2e-5.  irope_scale_q is bit-exact
(fp32 multiply, one round-to-nearest-even).  Dropping the temperature moves the result by rel_err 0.58 at
attn_scale 0.5 / floor_scale 16 and by 0.038 at the defaults around position 8191, so a kernel that ignores it fails
every attention case."""

from __future__ import annotations

import functools
import json

import numpy as np
import pytest

from oracle import cpu_ref as O
from tests import llama4_ref as R
from tests.conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

BAR = 1e-2


def _dev(x, dtype="bf16"):
    from pygpukit_amd.core import from_numpy

    x = np.ascontiguousarray(x, np.float32)
    return from_numpy(O.f32_to_bf16_bits(x) if dtype == "bf16" else x.astype(np.float16 if dtype == "f16" else np.float32))


def _host(a) -> np.ndarray:
    h = a.to_numpy()
    return O.bf16_bits_to_f32(h) if h.dtype == np.uint16 else h.astype(np.float32)


def _nan_out(shape, dtype="bf16"):
    from pygpukit_amd.core import from_numpy

    if dtype == "bf16":
        return from_numpy(np.full(shape, 0x7FC0, np.uint16))     # NaN everywhere: every element must be written
    return from_numpy(np.full(shape, np.nan, np.float16 if dtype == "f16" else np.float32))


def _pos(p, dtype=np.int64):
    from pygpukit_amd.core import from_numpy

    return from_numpy(np.ascontiguousarray(p, dtype))


def _round(x, dtype):
    return R.bf16_round(x) if dtype == "bf16" else x.astype(np.float16).astype(np.float32)


# ---- sdpa_irope --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _case(hq, hkv, q_len, kv_len, offset, pos0, d=128, dtype="bf16", attn_scale=0.5, floor_scale=16.0):
    rng = np.random.default_rng(1000 * q_len + kv_len + d)
    q, k, v = (_round(rng.standard_normal(s).astype(np.float32), dtype) for s in ((hq, q_len, d), (hkv, kv_len, d), (hkv, kv_len, d)))
    pos = np.arange(pos0, pos0 + q_len, dtype=np.int64)
    want = R.sdpa_irope(q, k, v, pos, attn_scale, floor_scale, offset)
    for a in (q, k, v, pos, want):
        a.setflags(write=False)
    return q, k, v, pos, want


def _run(q, k, v, pos, attn_scale, floor_scale, offset, dtype="bf16", pos_dtype=np.int64):
    from pygpukit_amd.ops.nn import sdpa_irope_strided

    hq, q_len, d = q.shape
    hkv, kv_len, _ = k.shape
    out = _nan_out(q.shape, dtype)
    sdpa_irope_strided(_dev(q, dtype), _dev(k, dtype), _dev(v, dtype), _pos(pos, pos_dtype), out, hq, hkv, q_len, kv_len, d,
                       (q_len * d, d), (kv_len * d, d), (q_len * d, d), attn_scale, floor_scale, offset)
    got = _host(out)
    assert np.isfinite(got).all()
    return got


CASES = [
    # hq, hkv, q_len, kv_len, offset, first position
    (4, 4, 200, 200, 0, 0),          # partial Q and KV tiles
    (4, 2, 200, 200, 0, 0),          # GQA
    (2, 2, 1, 70, 69, 69),           # decode row
    (8, 8, 129, 333, 204, 204),      # prefix, one-row second tile
    (2, 1, 512, 512, 0, 0),          # two KV runs
    (2, 1, 600, 1100, 500, 500),     # four KV runs and merge
    (2, 2, 70, 200, 0, 0),           # keys beyond the diagonal never seen
    (2, 2, 200, 70, 0, 0),           # kv_len < q_len, late rows see all
    (2, 2, 70, 70, 70, 0),           # offset >= kv_len: no masking
]


@pytest.mark.parametrize("hq,hkv,q_len,kv_len,offset,pos0", CASES)
def test_sdpa_irope_matches_the_restatement(hq, hkv, q_len, kv_len, offset, pos0):
    q, k, v, pos, want = _case(hq, hkv, q_len, kv_len, offset, pos0)
    err = rel_err(_run(q, k, v, pos, 0.5, 16.0, offset), want)
    print(f"sdpa_irope {(hq, hkv, q_len, kv_len)} offset {offset}: rel_err {err:.3e}")
    assert err <= BAR


def test_sdpa_irope_head_dim_64_float16():
    q, k, v, pos, want = _case(4, 2, 200, 200, 0, 0, d=64, dtype="f16")
    err = rel_err(_run(q, k, v, pos, 0.5, 16.0, 0, dtype="f16"), want)
    print(f"sdpa_irope D 64 f16: rel_err {err:.3e}")
    assert err <= BAR


def test_sdpa_irope_default_scales_with_the_step_at_8191_inside_a_tile():
    q, k, v, pos, want = _case(4, 4, 200, 200, 0, 8100, attn_scale=0.1, floor_scale=8192.0)
    t = R.irope_temperature(pos)
    assert t[0] == 1.0 and t[-1] > 1.0 and t[90] == 1.0 and t[91] > 1.0         # pos 8191 is row 91
    from pygpukit_amd.ops.nn import sdpa_irope

    out = sdpa_irope(_dev(q), _dev(k), _dev(v), _pos(pos))                        # the reference's signature, defaults
    got = _host(out)
    assert out.shape == q.shape and np.isfinite(got).all()
    err = rel_err(got, want)
    print(f"sdpa_irope defaults, positions 8100..8299: rel_err {err:.3e}")
    assert err <= BAR


def test_sdpa_irope_int32_positions():
    q, k, v, pos, want = _case(8, 8, 129, 333, 204, 204)
    err = rel_err(_run(q, k, v, pos, 0.5, 16.0, 204, pos_dtype=np.int32), want)
    print(f"sdpa_irope int32 positions: rel_err {err:.3e}")
    assert err <= BAR


def test_the_temperature_is_really_applied():
    q, k, v, pos, want = _case(4, 4, 200, 200, 0, 0)
    got = _run(q, k, v, np.zeros_like(pos), 0.5, 16.0, 0)
    err = rel_err(got, want)
    print(f"all positions zero against the real-positions oracle: rel_err {err:.3e}")
    assert err >= 1e-1
    assert rel_err(got, R.sdpa_irope(q, k, v, np.zeros_like(pos), 0.5, 16.0, 0)) <= BAR


def test_strided_entry_with_q_and_out_in_shd_layout():
    from pygpukit_amd.ops.nn import sdpa_irope_strided

    hq, hkv, q_len, kv_len = 4, 2, 200, 200
    q, k, v, pos, want = _case(hq, hkv, q_len, kv_len, 0, 0)
    out = _nan_out((q_len, hq, 128))
    sdpa_irope_strided(_dev(q.transpose(1, 0, 2)), _dev(k), _dev(v), _pos(pos), out, hq, hkv, q_len, kv_len, 128,
                       (128, hq * 128), (kv_len * 128, 128), (128, hq * 128), 0.5, 16.0, 0)
    shd = _host(out).transpose(1, 0, 2)
    assert np.isfinite(shd).all()
    np.testing.assert_array_equal(shd, _run(q, k, v, pos, 0.5, 16.0, 0))          # equals the contiguous result
    assert rel_err(shd, want) <= BAR


# ---- l2norm ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 128), (1030, 128), (7, 64), (5, 40), (3, 5, 4096)])
@pytest.mark.parametrize("dtype,bar", [("bf16", BAR), ("f32", 2e-5)])
def test_l2norm(shape, dtype, bar):
    from pygpukit_amd.ops.nn import l2norm

    rng = np.random.default_rng(sum(shape))
    x = rng.standard_normal(shape).astype(np.float32) * np.float32(3.0)
    x = _round(x, dtype) if dtype == "bf16" else x
    want = R.l2norm(x, 1e-5)
    xd = _dev(x, dtype)
    fresh = l2norm(xd, 1e-5)
    assert fresh.shape == tuple(shape) and fresh.dtype == xd.dtype
    given = _nan_out(shape, dtype)
    assert l2norm(xd, 1e-5, out=given) is given
    assert l2norm(xd, 1e-5, out=xd) is xd                                         # in place
    for name, a in (("fresh", fresh), ("out=", given), ("in place", xd)):
        got = _host(a)
        assert np.isfinite(got).all(), name
        err = rel_err(got, want)
        print(f"l2norm {shape} {dtype} {name}: rel_err {err:.3e}")
        assert err <= bar, name
    np.testing.assert_array_equal(_host(fresh), _host(given))
    np.testing.assert_array_equal(_host(fresh), _host(xd))


def test_l2norm_default_eps_matches_the_recorded_reference():
    from pygpukit_amd.ops.nn import l2norm

    g = load_golden("g7_llama4.npz")
    got = _host(l2norm(_dev(g["l2norm_a_x"], "f32")))
    assert rel_err(got, g["l2norm_a_y"]) <= 2e-5


# ---- irope_scale_q -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pos_dtype", [np.int64, np.int32])
def test_irope_scale_q_is_bit_exact(pos_dtype):
    from pygpukit_amd.ops.nn import irope_scale_q

    rng = np.random.default_rng(300)
    q = R.bf16_normal(rng, (300, 3, 128))
    pos = np.arange(300) * 29 + 5                                                 # steps 0 .. 541 of floor_scale 16
    out = irope_scale_q(_dev(q), _pos(pos, pos_dtype), 0.5, 16.0)
    assert out.shape == (300, 3, 128)
    want = O.f32_to_bf16_bits(R.irope_scale_q(q, pos, 0.5, 16.0))
    got = out.to_numpy()
    bad = np.argwhere(got != want)
    assert bad.size == 0, [(tuple(i), hex(got[tuple(i)]), hex(want[tuple(i)])) for i in bad[:8]]
    assert len(set(R.irope_temperature(pos, 0.5, 16.0).tolist())) > 100


def test_irope_scale_q_default_scales_and_float16():
    from pygpukit_amd.ops.nn import irope_scale_q

    rng = np.random.default_rng(301)
    q = rng.standard_normal((40, 2, 20)).astype(np.float16)          # head_dim % 8 != 0: the element-wise path
    pos = np.arange(8180, 8220)
    out = irope_scale_q(_dev(q, "f16"), _pos(pos))
    want = R.irope_scale_q(q.astype(np.float32), pos).astype(np.float16)
    np.testing.assert_array_equal(out.to_numpy(), want)


# ---- model -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _tiny_model():
    from pygpukit_amd.core import from_numpy
    from pygpukit_amd.llm.models.llama4 import Llama4Attention, Llama4Block, Llama4Config, Llama4MLP, Llama4Model

    g = load_golden("g7_llama4.npz")
    w = R.make_llama4_weights(R.TINY_CFG, int(g["model_seed"]))
    assert abs(R.checksum(w) - float(g["model_weight_checksum"])) <= 1e-5
    cfg = Llama4Config(**R.TINY_CFG)
    W = lambda a: from_numpy(O.f32_to_bf16_bits(a))          # noqa: E731  (weights are bf16-representable: exact)
    blocks = [Llama4Block(Llama4Attention(W(lw["q"]), W(lw["k"]), W(lw["v"]), W(lw["o"]), cfg),
                          Llama4MLP(W(lw["gate"]), W(lw["up"]), W(lw["down"])), W(lw["input_norm"]), W(lw["post_norm"]), cfg.rms_norm_eps)
              for lw in w["layers"]]
    return Llama4Model(cfg, W(w["embed"]), blocks, W(w["norm"]), W(w["lm_head"])), w, g


def test_tiny_model_logits_match_the_recorded_reference():
    model, _, g = _tiny_model()
    logits = model.forward(g["model_prompt"])
    assert logits.shape == (12, 100)
    got = _host(logits)
    assert np.isfinite(got).all()
    err = rel_err(got, g["model_logits"])
    print(f"tiny Llama-4 prefill logits: rel_err {err:.3e}")
    assert err <= BAR


def test_tiny_model_generates_the_recorded_tokens():
    from pygpukit_amd.llm.models.llama4 import generate

    model, _, g = _tiny_model()
    ids = generate(model, g["model_prompt"], max_new_tokens=6, eos_token_id=-1)
    assert ids.dtype == np.int64
    np.testing.assert_array_equal(ids[:12], g["model_prompt"])
    np.testing.assert_array_equal(ids[12:], g["model_tokens"])
    # eos stops the loop after the token is appended
    eos = int(g["model_tokens"][1])
    stop = generate(model, g["model_prompt"], max_new_tokens=6, eos_token_id=[eos])
    np.testing.assert_array_equal(stop[12:], g["model_tokens"][:list(g["model_tokens"]).index(eos) + 1])


def test_from_safetensors_round_trip(tmp_path):
    from pygpukit_amd.llm.models.llama4 import Llama4Model
    from pygpukit_amd.llm.safetensors import save_safetensors

    model, w, g = _tiny_model()
    (tmp_path / "config.json").write_text(json.dumps({"model_type": "llama4", "text_config": R.TINY_CFG}))
    save_safetensors(str(tmp_path / "model.safetensors"), {n: (O.f32_to_bf16_bits(a), "BF16") for n, a in R.hf_tensors(w).items()})
    loaded = Llama4Model.from_safetensors(tmp_path)
    assert loaded.config.floor_scale == 4.0 and len(loaded.blocks) == 2
    got = loaded.forward(g["model_prompt"]).to_numpy()
    np.testing.assert_array_equal(got, model.forward(g["model_prompt"]).to_numpy())
    assert rel_err(O.bf16_bits_to_f32(got), g["model_logits"]) <= BAR


# ---- refused cases -----------------------------------------------------------------------------------------------------

def test_refused_cases():
    from pygpukit_amd import _hip
    from pygpukit_amd.core import from_numpy
    from pygpukit_amd.ops.nn import irope_scale_q, l2norm, sdpa_irope, sdpa_irope_strided

    bf = lambda *s: from_numpy(np.zeros(s, np.uint16))       # noqa: E731
    f32 = lambda *s: from_numpy(np.zeros(s, np.float32))     # noqa: E731
    pos = lambda n: from_numpy(np.arange(n, dtype=np.int64))  # noqa: E731
    with pytest.raises(ValueError):
        sdpa_irope(f32(2, 8, 128), f32(2, 8, 128), f32(2, 8, 128), pos(8))                     # float32
    with pytest.raises(ValueError, match="head_dim"):
        sdpa_irope(bf(2, 8, 96), bf(2, 8, 96), bf(2, 8, 96), pos(8))
    with pytest.raises(ValueError, match="n_heads"):
        sdpa_irope(bf(3, 8, 128), bf(2, 8, 128), bf(2, 8, 128), pos(8))
    with pytest.raises(ValueError, match="causal_offset"):
        sdpa_irope(bf(2, 8, 128), bf(2, 8, 128), bf(2, 8, 128), pos(8), causal_offset=-1)
    with pytest.raises(ValueError, match="positions"):
        sdpa_irope(bf(2, 8, 128), bf(2, 8, 128), bf(2, 8, 128), pos(7))
    with pytest.raises(ValueError, match="positions"):
        sdpa_irope(bf(2, 8, 128), bf(2, 8, 128), bf(2, 8, 128), f32(8))
    with pytest.raises(ValueError):
        sdpa_irope(bf(2, 8, 128), bf(2, 8, 128), from_numpy(np.zeros((2, 8, 128), np.float16)), pos(8))
    with pytest.raises(ValueError):
        sdpa_irope(bf(8, 128), bf(2, 8, 128), bf(2, 8, 128), pos(8))
    with pytest.raises(ValueError, match="multiples of 8"):
        sdpa_irope_strided(bf(2, 8, 128), bf(2, 8, 128), bf(2, 8, 128), pos(8), bf(2, 8, 128), 2, 2, 8, 8, 128, (1028, 128), (1024, 128), (1024, 128))
    with pytest.raises(ValueError):
        irope_scale_q(bf(8, 128), pos(8))
    with pytest.raises(ValueError, match="positions"):
        irope_scale_q(bf(8, 2, 128), pos(9))
    with pytest.raises(ValueError):
        l2norm(from_numpy(np.zeros((4, 8), np.int32)))
    with pytest.raises(ValueError):
        l2norm(bf(4, 8), out=bf(4, 9))
    # the native entry refuses the same on its own, with a message
    x, o, p = bf(2, 8, 128), bf(2, 8, 128), pos(8)
    I64, BF16, F32 = p.dtype.code, x.dtype.code, f32(1).dtype.code

    def native(hq=2, hkv=2, d=128, offset=0, qs_h=1024, pos_dt=I64, dt=BF16):
        _hip.call("pgk_sdpa_irope", x._p, x._p, x._p, p._p, o._p, hq, hkv, 8, 8, d, 0.1, 8192.0, offset, qs_h, 128, 1024, 128, 1024, 128,
                  pos_dt, dt, None)

    with pytest.raises(RuntimeError, match="float16 / bfloat16 only"):
        native(dt=F32)
    with pytest.raises(RuntimeError, match="head_dim must be 64 or 128"):
        native(d=96)
    with pytest.raises(RuntimeError, match="n_heads mismatch"):
        native(hq=3)
    with pytest.raises(RuntimeError, match="causal_offset must be >= 0"):
        native(offset=-1)
    with pytest.raises(RuntimeError, match="multiples of 8"):
        native(qs_h=1028)
    with pytest.raises(RuntimeError, match="int64 or int32"):
        native(pos_dt=F32)
    native()          # and accepts the valid call
