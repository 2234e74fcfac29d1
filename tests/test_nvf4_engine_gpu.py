"""GPU tests of the engine's NVF4 weights (weight_format "nvf4", w4a16): the NK quantiser bit for bit, the tiny model
against the oracle on the dequantised weights, and the NVF4 engine against a bf16 engine built on the SAME dequantised
weights (dequantisation is exact in bf16, so the two differ only in accumulation order): prefill at every branch,
greedy decode, batches, captured graphs, in-graph sampling, memory and the error paths."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from oracle import cpu_ref as O
from tests import nvf4_engine_ref as NE
from tests.conftest import load_golden, rel_err
from tests.golden_cfg import TINY

pytestmark = pytest.mark.gpu

pk = pytest.importorskip("pygpukit_amd")
from pygpukit_amd import _hip, ops  # noqa: E402
from pygpukit_amd.core import from_numpy  # noqa: E402
from pygpukit_amd.core.array import GPUArray  # noqa: E402
from pygpukit_amd.core.dtypes import uint8  # noqa: E402
from pygpukit_amd.llm import synthetic as S  # noqa: E402
from pygpukit_amd.llm.engine import Engine  # noqa: E402

g3 = load_golden("g3_tiny_qwen3.npz")
PROMPT = [int(t) for t in g3["prompt"]]


def bits(x: np.ndarray) -> np.ndarray:
    return O.f32_to_bf16_bits(np.ascontiguousarray(x, np.float32))


# ---------------------------------------------------------------------------------------------------- 1. quantiser
@pytest.mark.parametrize("N,K", [(1, 32), (13, 96), (200, 1056), (1024, 3072), (37, 4096)])
def test_quantize_nk_bit_exact(N, K):
    rng = np.random.default_rng(N * 7 + K)
    w = NE.bf16_round(rng.standard_normal((N, K)).astype(np.float32) *
                      np.repeat(np.exp2(rng.integers(-30, 12, (N, K // 32))).astype(np.float32), 32, axis=1))
    wb = bits(w)
    if N >= 2 and K >= 64:
        wb[1, 3], wb[1, 40], wb[N - 1, K - 1] = 0x7FC0, 0x7F80, 0xFF80          # NaN, +inf, -inf
        wb[0, :32] = bits(np.array([6.0, 1.25, -1.25, 0.25, 0.75, 1.75, 2.5, 3.5, 5.0] + [0.0] * 23, np.float32))   # ties
        wb[0, 32:64] = bits(np.full(32, 2.0 ** -28, np.float32))                # a block under 1e-8
    data = GPUArray((N, K // 2), uint8)
    scale = GPUArray((N, K // 32), uint8)
    ops.quantize_bf16_to_nvf4_nk(from_numpy(wb), data, scale)
    got_d, got_s = data.to_numpy(), scale.to_numpy()
    wf = O.bf16_bits_to_f32(wb)
    want_d, want_s = NE.quantize_nk(wf)
    np.testing.assert_array_equal(got_s, want_s)
    np.testing.assert_array_equal(got_d, want_d)
    # the reference-layout device quantiser on W^T, transposed
    ref_d = GPUArray((K // 2, N), uint8)
    ref_s = GPUArray((K // 32, N), uint8)
    ops.quantize_bf16_to_nvf4(from_numpy(np.ascontiguousarray(wb.T)), ref_d, ref_s)
    np.testing.assert_array_equal(got_d, ref_d.to_numpy().T)
    np.testing.assert_array_equal(got_s, ref_s.to_numpy().T)


def test_quantize_nk_interface_errors():
    w = from_numpy(bits(np.zeros((4, 48), np.float32)))
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.quantize_bf16_to_nvf4_nk(w, GPUArray((4, 24), uint8), GPUArray((4, 2), uint8))
    w = from_numpy(bits(np.zeros((4, 64), np.float32)))
    with pytest.raises(ValueError, match="too small"):
        ops.quantize_bf16_to_nvf4_nk(w, GPUArray((4, 16), uint8), GPUArray((4, 2), uint8))


# ---------------------------------------------------------------------------------------------------- helpers
def _b16(x):
    return from_numpy(bits(x))


def build_pair(cfg: dict, w: dict, *, max_seq_len: int, max_batch: int, use_qk_norm: bool = True):
    """(NVF4 engine, bf16 engine on the dequantised weights, NVF4 layer dicts).  The fused matrices are quantised on the
    device; the bf16 engine gets code x scale of exactly those bytes."""
    embed, fnorm = _b16(w["embed"]), _b16(w["final_norm"])
    nv, deq = [], []
    for lw in w["layers"]:
        norms = {"attn_norm": _b16(lw["attn_norm"]), "mlp_norm": _b16(lw["mlp_norm"]),
                 "q_norm": _b16(lw["q_norm"]) if use_qk_norm else None, "k_norm": _b16(lw["k_norm"]) if use_qk_norm else None}
        a, b = dict(norms), dict(norms)
        for name in ("w_qkv", "w_o", "w_gate_up", "w_down"):
            d, s = ops.quantize_nvf4_nk(_b16(lw[name]))
            a[name], a["s" + name[1:]] = d, s
            b[name] = _b16(NE.dequant_nk(d.to_numpy(), s.to_numpy()))
        nv.append(a)
        deq.append(b)
    kw = dict(max_seq_len=max_seq_len, max_batch=max_batch, use_qk_norm=use_qk_norm)
    return Engine(cfg, embed, nv, fnorm, None, weight_format="nvf4", **kw), Engine(cfg, embed, deq, fnorm, None, weight_format="bf16", **kw), nv


def eager_greedy(eng: Engine, prompt, n: int):
    """prefill + n eager decode steps; (tokens, per-step logits)."""
    lg = eng.prefill(prompt)
    tok, toks, logits = int(np.argmax(lg)), [], []
    eng.set_state([tok], [len(prompt)])
    for _ in range(n):
        eng.decode_step(1)
        eng.synchronize()
        row = eng.logits(1).to_numpy()[0].copy()
        logits.append(row)
        tok = int(np.argmax(row))
        toks.append(tok)
    return toks, logits


# ---------------------------------------------------------------------------------------------------- 2. tiny vs oracle
def test_tiny_engine_nvf4_vs_oracle():
    tiny = O.make_qwen3_weights(TINY, seed=int(g3["seed"]), bf16=True)
    wq = {"embed": tiny["embed"], "final_norm": tiny["final_norm"], "layers": []}
    for lw in tiny["layers"]:
        d = dict(lw)
        for names in (("q", "k", "v"), ("o",), ("gate", "up"), ("down",)):
            fused = np.concatenate([lw[n] for n in names], axis=0)
            deq = NE.dequant_nk(*NE.quantize_nk(fused))
            r = 0
            for n in names:
                d[n] = deq[r:r + lw[n].shape[0]]
                r += lw[n].shape[0]
        wq["layers"].append(d)
    ref = O.build_qwen3_ref(TINY, wq, max_pos=128)
    want, want_logits = ref.generate(PROMPT, max_new_tokens=6, temperature=0.0, top_k=0, top_p=1.0, return_logits=True)
    eng = S.build_engine_from_weights(TINY, tiny, max_seq_len=128, max_batch=1, weight_format="nvf4")
    got = eng.generate_greedy(PROMPT, max_new_tokens=6)
    assert rel_err(eng.last_prefill_logits, want_logits[0]) < 1e-2
    q_err_oracle = rel_err(want_logits[0], g3["step_logits"][0])
    q_err_gpu = rel_err(eng.last_prefill_logits, g3["step_logits"][0])
    assert q_err_gpu < 1.1 * q_err_oracle + 1e-3, (q_err_gpu, q_err_oracle)
    assert got == want


# ---------------------------------------------------------------------------------------------------- 3. real widths
QWEN_W = dict(vocab_size=4096, hidden_size=1024, num_layers=2, num_heads=16, num_kv_heads=8, head_dim=128,
              intermediate_size=3072, norm_eps=1e-6, rope_theta=1e6)
D64_W = dict(vocab_size=4096, hidden_size=2048, num_layers=2, num_heads=16, num_kv_heads=4, head_dim=64,
             intermediate_size=4096, norm_eps=1e-5, rope_theta=5e5)


@pytest.mark.parametrize("cfg", [QWEN_W, D64_W], ids=["qwen3_0.6b_widths", "head_dim64"])
def test_real_widths_vs_dequantised_bf16_engine(cfg):
    w = NE.random_engine_weights(cfg, seed=11)
    eng, ref, _ = build_pair(cfg, w, max_seq_len=2048 + 24, max_batch=1, use_qk_norm=cfg["head_dim"] == 128)
    rng = np.random.default_rng(5)
    for n in (1, 37, 128, 129, 300, 2048):
        prompt = rng.integers(0, cfg["vocab_size"], n).tolist()
        a, b = eng.prefill(prompt), ref.prefill(prompt)
        assert rel_err(a, b) < 1e-2, (n, rel_err(a, b))
    prompt = rng.integers(0, cfg["vocab_size"], 40).tolist()
    ta, la = eager_greedy(eng, prompt, 16)
    tb, lb = eager_greedy(ref, prompt, 16)
    assert ta == tb
    for x, y in zip(la, lb):
        assert rel_err(x, y) < 1e-2


# ---------------------------------------------------------------------------------------------------- 4. batches
def test_batches_match_single_sequences():
    cfg = dict(TINY, vocab_size=2048)
    w = NE.random_engine_weights(cfg, seed=4)
    eng, _, nv = build_pair(cfg, w, max_seq_len=96, max_batch=11)
    solo = Engine(cfg, _b16(w["embed"]), nv, _b16(w["final_norm"]), None, max_seq_len=96, max_batch=1, weight_format="nvf4")
    rng = np.random.default_rng(9)
    prompts = [rng.integers(0, cfg["vocab_size"], 3 + 5 * b).tolist() for b in range(11)]
    nxt = [int(t) for t in rng.integers(0, cfg["vocab_size"], 11)]
    pos = [len(p) for p in prompts]
    want = []
    for b in range(11):
        solo.prefill(prompts[b])
        solo.set_state([nxt[b]], [pos[b]])
        solo.decode_step(1)
        solo.synchronize()
        want.append(solo.logits(1).to_numpy()[0].copy())
    for b in range(11):
        eng.prefill(prompts[b], seq=b)
    for B in (1, 2, 3, 4, 8, 11):
        eng.set_state(nxt[:B], pos[:B])      # the step rewrites the same KV row with the same values each time
        eng.decode_step(B)
        eng.synchronize()
        got = eng.logits(B).to_numpy()
        for b in range(B):
            assert rel_err(got[b], want[b]) < 1e-2, (B, b, rel_err(got[b], want[b]))


# ---------------------------------------------------------------------------------------------------- 5. graphs, sampling
@pytest.mark.parametrize("plen", [20, 600], ids=["short_ctx", "long_ctx"])
def test_graph_replay_equals_eager(plen):
    cfg = dict(TINY, vocab_size=2048)
    w = NE.random_engine_weights(cfg, seed=6)
    eng, _, _ = build_pair(cfg, w, max_seq_len=1024, max_batch=1)
    prompt = np.random.default_rng(plen).integers(0, cfg["vocab_size"], plen).tolist()
    first = int(np.argmax(eng.prefill(prompt)))
    eng.set_state([first], [plen])
    eng.reset_log()
    for _ in range(8):
        eng.decode_step(1)
    eng.synchronize()
    eager = eng.read_tokens(1, 8)[:, 0].tolist()
    eager_logits = eng.logits(1).to_numpy()[0].copy()
    assert eng.launches_per_step() > 0
    eng.prefill(prompt)
    eng.set_state([first], [plen])
    eng.reset_log()
    eng.capture(1)
    eng.replay(8)
    eng.synchronize()
    assert eng.read_tokens(1, 8)[:, 0].tolist() == eager
    assert rel_err(eng.logits(1).to_numpy()[0], eager_logits) < 1e-5


def test_in_graph_sampling_matches_dequantised_bf16():
    cfg = dict(TINY, vocab_size=2048)
    w = NE.random_engine_weights(cfg, seed=8, std=0.06, embed_std=0.05)   # the layers, not the token's own embedding, lead
    eng, ref, _ = build_pair(cfg, w, max_seq_len=128, max_batch=1)
    prompt = np.random.default_rng(2).integers(0, cfg["vocab_size"], 12).tolist()
    u = np.random.default_rng(7).random((12, 1), dtype=np.float32)
    out = []
    for e in (eng, ref):
        first = int(np.argmax(e.prefill(prompt)))
        e.set_sampling(1.0, top_k=8, top_p=1.0, uniforms=u)
        e.set_state([first], [len(prompt)])
        e.reset_log()
        e.capture(1)
        e.replay(12)
        e.synchronize()
        out.append(e.read_tokens(1, 12)[:, 0].tolist())
        e.set_sampling(0.0)
    assert out[0] == out[1], out
    assert len(set(out[0])) > 1, out


# ---------------------------------------------------------------------------------------------------- 6. memory
def test_workspace_does_not_grow_with_layers():
    ws = {}
    for L in (2, 4):
        cfg = dict(QWEN_W, num_layers=L, vocab_size=1024)
        w = NE.random_engine_weights(cfg, seed=1)
        eng, _, nv = build_pair(cfg, w, max_seq_len=64, max_batch=1)
        eng.prefill([1, 2, 3])
        ws[L] = eng.bytes()[1]
        if L == 2:
            nv_bytes = sum(a.size for lw in nv for k, a in lw.items() if k[:2] in ("w_", "s_"))
            bf_bytes = 2 * sum(n * k for n, k in NE.layer_shapes(cfg).values()) * L
            assert nv_bytes <= 0.27 * bf_bytes, (nv_bytes, bf_bytes)
    assert ws[2] == ws[4], ws


# ---------------------------------------------------------------------------------------------------- 7. errors
def _raw_create(cfg: dict, layers: list[dict], weight_format: int, embed: GPUArray, fnorm: GPUArray):
    mc = _hip.ModelConfig(cfg["vocab_size"], cfg["hidden_size"], cfg["num_layers"], cfg["num_heads"], cfg["num_kv_heads"],
                          cfg["head_dim"], cfg["intermediate_size"], 64, 1, float(cfg["norm_eps"]), float(cfg["rope_theta"]),
                          weight_format, 0)
    arr = (_hip.LayerWeights * len(layers))()
    for i, lw in enumerate(layers):
        for name, _ in _hip.LayerWeights._fields_:
            t = lw.get(name)
            setattr(arr[i], name, t.data_ptr() if t is not None else None)
    h = C.c_void_p()
    _hip.call("pgk_engine_create", C.byref(mc), embed._p, None, fnorm._p, arr, C.byref(h))
    _hip.call("pgk_engine_destroy", h)


def test_native_create_rejects_bad_nvf4_engines():
    cfg = dict(TINY, vocab_size=256)
    w = NE.random_engine_weights(cfg, seed=2)
    _, _, nv = build_pair(cfg, w, max_seq_len=64, max_batch=1, use_qk_norm=False)
    embed, fnorm = _b16(w["embed"]), _b16(w["final_norm"])
    _raw_create(cfg, nv, 3, embed, fnorm)                                   # the good one is accepted
    no_scales = [dict(lw, s_o=None) for lw in nv]
    with pytest.raises(_hip.PgkError, match="missing its scales o"):
        _raw_create(cfg, no_scales, 3, embed, fnorm)
    odd = dict(cfg, hidden_size=192, num_heads=3, num_kv_heads=1)
    w2 = NE.random_engine_weights(odd, seed=2)
    lay = [{k: (_b16(v) if k.endswith("norm") else None) for k, v in lw.items()} for lw in w2["layers"]]
    for lw, src in zip(lay, w2["layers"]):
        for name in ("w_qkv", "w_o", "w_gate_up", "w_down"):
            lw[name], lw["s" + name[1:]] = ops.quantize_nvf4_nk(_b16(src[name]))
    with pytest.raises(_hip.PgkError, match="multiples of 128"):
        _raw_create(odd, lay, 3, _b16(w2["embed"]), _b16(w2["final_norm"]))
    with pytest.raises(ValueError, match="multiples of 128"):
        Engine(odd, _b16(w2["embed"]), lay, _b16(w2["final_norm"]), weight_format="nvf4")


def test_model_build_engine_nvf4():
    from pygpukit_amd.llm.decode.batch import DecodeBatch
    from pygpukit_amd.llm.decode.m1_graph import DecodeM1Graph

    tiny = O.make_qwen3_weights(TINY, seed=int(g3["seed"]), bf16=True)
    model = S.build_model_from_weights(TINY, tiny, dtype="bfloat16", max_pos=128)
    eng = model.build_engine(max_seq_len=128, weight_format="nvf4")
    assert eng.weight_format == "nvf4"
    want = S.build_engine_from_weights(TINY, tiny, max_seq_len=128, max_batch=1, weight_format="nvf4").generate_greedy(PROMPT, 6)
    assert eng.generate_greedy(PROMPT, 6) == want
    assert model.build_engine(max_seq_len=64).weight_format == "bf16"          # the default is unchanged
    m1 = DecodeM1Graph()
    m1.bind(model)
    m1.init_graph(max_seq_len=64, weight_format="nvf4")
    assert m1.engine.weight_format == "nvf4"
    db = DecodeBatch(batch_size=2)
    db.bind(model)
    db.init_graph(max_seq_len=64, weight_format="nvf4")
    assert db.engine.weight_format == "nvf4"
    # models it cannot take
    f32_model = S.build_model_from_weights(TINY, tiny, dtype="float32", max_pos=128)
    with pytest.raises(NotImplementedError, match="bfloat16"):
        f32_model.build_engine(weight_format="nvf4")
    odd = dict(TINY, hidden_size=192, num_heads=3, num_kv_heads=1)
    odd_model = S.build_model_from_weights(odd, O.make_qwen3_weights(odd, seed=1, bf16=True), dtype="bfloat16", max_pos=64)
    with pytest.raises(ValueError, match="multiples of 128"):
        odd_model.build_engine(weight_format="nvf4")
