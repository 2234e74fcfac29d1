"""GPU tests of the Mixture-of-Experts path (ops_moe.hip through pygpukit_amd.ops, ops.matmul.grouped and
llm.layers.MoELayer) against the restated oracle of tests/moe_ref.py: routing bit for bit, grouped GEMMs bit for bit on
exact small-integer data and at 1e-2 on random data, MoELayer at the Mixtral and Qwen3-30B-A3B shapes, repeatability,
graph replay with different routing, and tiny Mixtral / Qwen3-MoE checkpoints end to end."""

from __future__ import annotations

import json

import numpy as np
import pytest

from oracle import cpu_ref as O
from tests import moe_ref as R
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu

pk = pytest.importorskip("pygpukit_amd")
from pygpukit_amd import ops  # noqa: E402
from pygpukit_amd.core import bfloat16, float32, from_numpy  # noqa: E402
from pygpukit_amd.core.array import GPUArray  # noqa: E402
from pygpukit_amd.core.dtypes import int32, uint8  # noqa: E402
from pygpukit_amd.llm.config import TransformerConfig  # noqa: E402
from pygpukit_amd.llm.layers import LinearFP8, MoELayer  # noqa: E402
from pygpukit_amd.llm import safetensors as ST  # noqa: E402


def dev(x, dt="bfloat16"):
    x = np.ascontiguousarray(x, dtype=np.float32)
    return from_numpy(x) if dt == "float32" else from_numpy(O.f32_to_bf16_bits(x).reshape(x.shape))


def host(a) -> np.ndarray:
    h = a.to_numpy()
    return O.bf16_bits_to_f32(h) if a.dtype == bfloat16 else h


def i32(x):
    return from_numpy(np.ascontiguousarray(x, dtype=np.int32))


def route(logits_dev, E, k):
    T = logits_dev.shape[0]
    w, idx = GPUArray((T, k), logits_dev.dtype), GPUArray((T, k), int32)
    ops.moe_topk_softmax(logits_dev, w, idx, k)
    return w, idx


def permute(idx_dev, E, k):
    T = idx_dev.shape[0]
    counts, offsets = GPUArray((E,), int32), GPUArray((E + 1,), int32)
    perm, rev = GPUArray((T * k,), int32), GPUArray((T * k,), int32)
    tiles = ops.moe_compute_permutation(idx_dev, counts, offsets, perm, rev, E, k)
    return counts, offsets, perm, rev, tiles


# ----------------------------------------------------------------------------------------------------- routing
@pytest.mark.parametrize("E, k, T", [(8, 2, 1), (8, 1, 37), (60, 8, 300), (128, 8, 1100), (256, 8, 700), (256, 2, 5000),
                                     (8, 8, 64)])
@pytest.mark.parametrize("dt", ["bfloat16", "float32"])
def test_routing_bit_exact(E, k, T, dt):
    rng = np.random.default_rng(E * 7 + k + T)
    logits = rng.standard_normal((T, E)).astype(np.float32)
    logits = np.round(logits * 4) / 4 if T > 1 else logits      # many exact ties
    logits[0, :] = 1.0                                           # a row of ties: experts 0..k-1
    if T > 3:
        logits[1, E // 2] = np.nan
        logits[2, :] = -np.inf
        logits[3, 1::2] = 5.0
    ld = dev(logits, dt)
    seen = host(ld)                                              # the values the kernel sees
    w, idx = route(ld, E, k)
    want_w, want_idx = R.topk_softmax(seen, k, bf16=dt == "bfloat16")
    np.testing.assert_array_equal(idx.to_numpy(), want_idx)
    got_w = host(w)      # expf against NumPy's exp: an fp32 ulp, so at most one bf16 ulp after rounding
    np.testing.assert_allclose(got_w, want_w, rtol=2e-6 if dt == "float32" else 2 ** -8, atol=0)
    # the two-step entries: values as given, then the in-place softmax
    v2, i2 = GPUArray((T, k), ld.dtype), GPUArray((T, k), int32)
    ops.moe_topk_with_indices(ld, v2, i2, k)
    np.testing.assert_array_equal(i2.to_numpy(), want_idx)
    np.testing.assert_array_equal(host(v2), np.take_along_axis(seen, want_idx, axis=1))
    ops.moe_softmax_topk(v2, k)
    np.testing.assert_array_equal(host(v2), got_w)

    counts, offsets, perm, rev, tiles = permute(idx, E, k)
    c, o, p, r = R.permutation(want_idx, E)
    np.testing.assert_array_equal(counts.to_numpy(), c)
    np.testing.assert_array_equal(offsets.to_numpy(), o)
    np.testing.assert_array_equal(perm.to_numpy(), p)
    np.testing.assert_array_equal(rev.to_numpy(), r)
    np.testing.assert_array_equal(tiles.to_numpy(), R.tile_table(o, T, k, E))


@pytest.mark.parametrize("T, k, E", [(1, 2, 8), (4100, 2, 8), (9000, 8, 128), (33, 4, 60)])
def test_permutation_one_expert_takes_all_and_invalid_ids(T, k, E):
    rng = np.random.default_rng(T)
    idx = rng.integers(0, E // 2, (T, k)).astype(np.int32)      # experts E/2 .. E-2 receive nothing
    idx[:, 0] = E - 1                                            # an expert that receives every token
    if T > 2:
        idx[1, 0] = -3                                           # ids outside [0, E) are not placed
        idx[2, -1] = E
    counts, offsets, perm, rev, tiles = permute(i32(idx), E, k)
    c, o, p, r = R.permutation(idx, E)
    assert (c == 0).any() and c[E - 1] >= T - 1
    for got, want in zip((counts, offsets, perm, rev), (c, o, p, r)):
        np.testing.assert_array_equal(got.to_numpy(), want)
    np.testing.assert_array_equal(tiles.to_numpy(), R.tile_table(o, T, k, E))
    ids = GPUArray((T * k,), int32)
    ops.moe_expand_expert_offsets(offsets, ids, E)
    np.testing.assert_array_equal(ids.to_numpy(), R.expand_offsets(o, T * k))
    x = np.random.default_rng(1).standard_normal((T, 72)).astype(np.float32)
    g = GPUArray((T * k, 72), bfloat16)
    ops.moe_gather(dev(x), perm, g, k)
    want = np.where((p >= 0)[:, None], O.bf16_round(x)[np.maximum(p, 0) // k], 0.0)
    np.testing.assert_array_equal(host(g), want)


def test_scatter_matches_oracle_and_sums_slabs():
    T, k, H, E = 19, 3, 200, 6
    rng = np.random.default_rng(5)
    idx = np.stack([rng.permutation(E)[:k] for _ in range(T)]).astype(np.int32)
    _, _, _, rev = R.permutation(idx, E)
    w = O.bf16_round(rng.random((T, k)).astype(np.float32))
    y = O.bf16_round(rng.standard_normal((T * k, H)).astype(np.float32))
    out = GPUArray((T, H), bfloat16)
    ops.moe_scatter(dev(y), dev(w), i32(rev), out, k)
    np.testing.assert_array_equal(host(out), O.bf16_round(R.scatter(y, w, rev, k)))
    slabs = rng.standard_normal((3, T * k, H)).astype(np.float32)
    ops.moe_scatter(dev(slabs, "float32"), dev(w), i32(rev), out, k)
    ysum = ((slabs[0] + slabs[1]).astype(np.float32) + slabs[2]).astype(np.float32)
    np.testing.assert_array_equal(host(out), O.bf16_round(R.scatter(ysum, w, rev, k)))


# ----------------------------------------------------------------------------------------------------- grouped GEMM
CODE = {0: 0x00, 1: 0x38, 2: 0x40, 3: 0x44, 4: 0x48}


def int_codes(v):
    c = np.vectorize(lambda x: CODE[abs(int(x))])(v).astype(np.uint8)
    return np.where(v < 0, c | 0x80, c).astype(np.uint8)


def experts_int(E, N, K, seed):
    """Small-integer weights, asymmetric (row 0 and column 0 ramps), different per expert."""
    rng = np.random.default_rng(seed)
    w = rng.integers(-3, 4, (E, N, K))
    w[:, 0, :] = np.arange(K) % 5 - 2
    w[:, :, 0] = (np.arange(N) % 4)[None, :]
    w[np.arange(E), 1, 1] = np.arange(E) % 4                      # a wrong expert stride cannot pass
    return w


def sorted_ids(T, k, E, seed, skew=False):
    rng = np.random.default_rng(seed)
    idx = np.stack([rng.permutation(E)[:k] for _ in range(T)]).astype(np.int32)
    if skew:
        idx[: T // 2, 0] = 0
        idx[: T // 2, 1:] = np.where(idx[: T // 2, 1:] == 0, 1, idx[: T // 2, 1:])
    return idx


def run_grouped(fp8, a_rows, wq, scale, **kw):
    if fp8:
        return ops.grouped_gemm_fp8_bf16(a_rows, wq, scale, kw.pop("ids", None), **kw)
    return ops.grouped_gemm_bf16(a_rows, wq, kw.pop("ids", None), **kw)


# (T, k, E, N, K): T*k/E about 1 (weight-streaming regime) and about 512 (tiled regime); segments not multiples of 128.
# The weight-streaming kernel holds 1, 2, 4 or 8 row tiles of 16 by T*k: 6 and 320 rows take 1 and 8; 24 rows take 2 (K = 1.5
# LDS tiles of 256) and 50 rows take 4 (K = 2.5 tiles).
SHAPES = [(3, 2, 8, 256, 384), (40, 8, 16, 384, 512), (2048, 2, 8, 256, 256), (700, 4, 5, 384, 640),
          (12, 2, 8, 128, 384), (25, 2, 8, 128, 640)]


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_grouped_gemm_bit_exact(fp8, shape):
    T, k, E, N, K = shape
    wi = experts_int(E, N, K, seed=T + N)
    a = np.random.default_rng(T).integers(-2, 3, (T, K)).astype(np.float32)
    if fp8:
        rng = np.random.default_rng(9)
        sexp = rng.integers(-3, 3, (E, N // 128, K // 128))
        sexp[:, 0, :] += np.arange(K // 128)[None, :] % 2           # scale stride errors change the result
        sbits = O.f32_to_bf16_bits(np.exp2(sexp).astype(np.float32))
        wq, scale = from_numpy(int_codes(wi)), from_numpy(sbits)
        wf = R.dequant_experts(int_codes(wi), sbits)
    else:
        wq, scale, wf = dev(wi.astype(np.float32)), None, wi.astype(np.float32)
    idx = sorted_ids(T, k, E, seed=N, skew=True)
    c, o, p, r = R.permutation(idx, E)
    ids = R.expand_offsets(o, T * k)
    want_sorted = R.grouped_gemm(a[p // k], wf, ids)
    _, offsets, perm, _, tiles = permute(i32(idx), E, k)
    # sorted entry on gathered rows, on x through the permutation, and as fp32 split-K slabs
    gathered = GPUArray((T * k, K), bfloat16)
    ops.moe_gather(dev(a), perm, gathered, k)
    got = run_grouped(fp8, gathered, wq, scale, tiles=tiles, expert_offsets=offsets)
    np.testing.assert_array_equal(host(got), O.bf16_round(want_sorted))
    got = run_grouped(fp8, dev(a), wq, scale, tiles=tiles, expert_offsets=offsets, permute_indices=perm, top_k=k)
    np.testing.assert_array_equal(host(got), O.bf16_round(want_sorted))
    slabs = run_grouped(fp8, gathered, wq, scale, tiles=tiles, expert_offsets=offsets, out_slabs=True)
    np.testing.assert_array_equal(host(slabs).sum(axis=0), want_sorted)
    # rows entry with the rows in any order
    shuf = np.random.default_rng(3).permutation(T * k)
    got = run_grouped(fp8, dev(a[p // k][shuf]), wq, scale, ids=i32(ids[shuf]))
    np.testing.assert_array_equal(host(got), O.bf16_round(want_sorted[shuf]))


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_grouped_gemm_random(fp8, shape):
    T, k, E, N, K = shape
    rng = np.random.default_rng(N + K)
    a = O.bf16_round(rng.standard_normal((T, K)).astype(np.float32))
    w = rng.standard_normal((E, N, K)).astype(np.float32) * 0.05
    if fp8:
        q = [O.quantize_fp8_e4m3_block(w[e]) for e in range(E)]
        codes, sbits = np.stack([c for c, _ in q]), np.stack([s for _, s in q])
        wq, scale, wf = from_numpy(codes), from_numpy(sbits), R.dequant_experts(codes, sbits)
    else:
        wq, scale, wf = dev(w), None, O.bf16_round(w)
    idx = sorted_ids(T, k, E, seed=K)
    _, o, p, _ = R.permutation(idx, E)
    ids = R.expand_offsets(o, T * k)
    want = R.grouped_gemm(a[p // k], wf, ids)
    _, offsets, perm, _, tiles = permute(i32(idx), E, k)
    got = run_grouped(fp8, dev(a), wq, scale, tiles=tiles, expert_offsets=offsets, permute_indices=perm, top_k=k)
    assert rel_err(host(got), want) < 1e-2
    got = run_grouped(fp8, dev(a[p // k]), wq, scale, ids=i32(ids))
    assert rel_err(host(got), want) < 1e-2


def test_grouped_interface_errors():
    a = GPUArray((4, 256), bfloat16)
    w8, s = GPUArray((2, 256, 256), uint8), GPUArray((2, 2, 2), bfloat16)
    ids = GPUArray((4,), int32)
    with pytest.raises(ValueError, match="requires 2D input"):
        ops.grouped_gemm_fp8_bf16(GPUArray((4,), bfloat16), w8, s, ids)
    with pytest.raises(ValueError, match="requires uint8"):
        ops.grouped_gemm_fp8_bf16(a, GPUArray((2, 256, 256), bfloat16), s, ids)
    with pytest.raises(ValueError, match="K mismatch"):
        ops.grouped_gemm_fp8_bf16(a, GPUArray((2, 256, 128), uint8), s, ids)
    with pytest.raises(ValueError, match="row_expert_ids size"):
        ops.grouped_gemm_fp8_bf16(a, w8, s, GPUArray((3,), int32))
    with pytest.raises(ValueError, match="num_experts=300"):
        ops.moe_topk_softmax(GPUArray((2, 300), bfloat16), GPUArray((2, 2), bfloat16), GPUArray((2, 2), int32), 2)
    with pytest.raises(ValueError, match="k=9"):
        ops.moe_topk_softmax(GPUArray((2, 16), bfloat16), GPUArray((2, 9), bfloat16), GPUArray((2, 9), int32), 9)


# ----------------------------------------------------------------------------------------------------- MoELayer
class LazyExperts:
    """Expert e's (gate, up, down) fp32 weights, built on demand from three shared bases (rows rolled per expert and
    scaled), so the real shapes need no gigabytes of host memory."""

    def __init__(self, E, I, H, seed, fp8):
        rng = np.random.default_rng(seed)
        self.E, self.fp8 = E, fp8
        if fp8:     # codes with exponent fields 5..9 and random mantissas; bf16 scales differ per expert and block
            self.base = [(rng.integers(0, 2, s) << 7 | rng.integers(5, 10, s) << 3 | rng.integers(0, 8, s)).astype(np.uint8)
                         for s in ((I, H), (I, H), (H, I))]
            self.sexp = [rng.integers(-14, -11, (E,) + (s[0] // 128, s[1] // 128)) for s in ((I, H), (I, H), (H, I))]
        else:
            self.base = [O.bf16_round(rng.standard_normal(s).astype(np.float32) * np.float32(0.03)) for s in ((I, H), (I, H), (H, I))]

    def raw(self, e):
        out = []
        for j, b in enumerate(self.base):
            m = np.roll(b, 37 * e + 11 * j, axis=0)
            if self.fp8:
                out.append((np.ascontiguousarray(m), O.f32_to_bf16_bits(np.exp2(self.sexp[j][e]).astype(np.float32))))
            else:
                out.append(np.ascontiguousarray(m * np.float32(2.0 ** -(e % 3))))
        return out

    def __getitem__(self, e):
        if self.fp8:
            return tuple(O.dequantize_fp8_e4m3_block(c, s) for c, s in self.raw(e))
        return tuple(self.raw(e))

    def device(self):
        if self.fp8:
            return [tuple(LinearFP8(from_numpy(c), from_numpy(s)) for c, s in self.raw(e)) for e in range(self.E)]
        return [tuple(dev(m) for m in self.raw(e)) for e in range(self.E)]


def router_gap_ok(logits, k):
    """Per row: the k-th and (k+1)-th logits differ by 0.05 and by 4 bf16 ulps of the row's largest magnitude, so
    neither the bf16 rounding of the router output nor a last-bit difference in its sum can swap them."""
    s = -np.sort(-np.asarray(logits, np.float64), axis=1)
    return s[:, k - 1] - s[:, k] >= np.maximum(0.05, 4 * 2.0 ** -8 * np.abs(s).max(axis=1))


def margin_tokens(gate, T, H, k, seed):
    """T bf16 rows of x whose router logits pass router_gap_ok."""
    rng = np.random.default_rng(seed)
    rows = []
    while len(rows) < T:
        x = O.bf16_round(rng.standard_normal((256, H)).astype(np.float32))
        rows += list(x[router_gap_ok(x @ gate.T, k)])
    return np.stack(rows[:T])


MIXTRAL = dict(H=4096, I=14336, E=8, k=2)
QWEN3_30B = dict(H=2048, I=768, E=128, k=8)


def make_layer(shape, fp8, seed):
    H, I, E, k = shape["H"], shape["I"], shape["E"], shape["k"]
    cfg = TransformerConfig(hidden_size=H, num_heads=16, num_layers=1, intermediate_size=I, num_experts=E,
                            num_experts_per_tok=k, moe_intermediate_size=I)
    gate = O.bf16_round(np.random.default_rng(seed).standard_normal((E, H)).astype(np.float32) * np.float32(0.01))
    ex = LazyExperts(E, I, H, seed + 1, fp8)
    return MoELayer(cfg, dev(gate), ex.device()), R.RefMoE(gate, ex, k), gate


@pytest.fixture(scope="module", params=[("mixtral", False), ("mixtral", True), ("qwen3", False), ("qwen3", True)],
                ids=["mixtral-bf16", "mixtral-fp8", "qwen3-bf16", "qwen3-fp8"])
def layer(request):
    name, fp8 = request.param
    shape = MIXTRAL if name == "mixtral" else QWEN3_30B
    moe, ref, gate = make_layer(shape, fp8, seed=len(name) + fp8)
    yield shape, moe, ref, gate
    del moe


@pytest.mark.parametrize("T", [1, 7, 300])
def test_moe_layer_matches_oracle(layer, T):
    shape, moe, ref, gate = layer
    H, k = shape["H"], shape["k"]
    x = margin_tokens(gate, T, H, k, seed=T)
    assert router_gap_ok(x @ gate.T, k).all()
    got = moe(dev(x))
    assert got.shape == (T, H)
    want = ref(x)
    assert rel_err(host(got), want) < 1e-2
    if T == 7:  # [B, S, H] input, and two runs give identical bytes
        again = moe(dev(x).reshape(1, T, H))
        assert again.shape == (1, T, H)
        np.testing.assert_array_equal(again.to_numpy().reshape(T, H), got.to_numpy())


def test_moe_layer_graph_replay_reroutes():
    """A captured forward re-routes on replay: no host synchronisation or host-sized launch inside it."""
    shape = dict(H=512, I=256, E=16, k=4)
    moe, ref, gate = make_layer(shape, False, seed=3)
    T = 24
    x1 = margin_tokens(gate, T, 512, 4, seed=1)
    x2 = margin_tokens(gate, T, 512, 4, seed=2)
    assert not np.array_equal(R.topk_indices(x1 @ gate.T, 4), R.topk_indices(x2 @ gate.T, 4))
    xd = dev(x1)
    moe(xd)                                      # warm the pool and the kernels outside the capture
    graph = pk.CudaGraph()
    graph.begin_capture()
    out = moe(xd)
    graph.end_capture()
    xd.copy_from_numpy(O.f32_to_bf16_bits(x2))
    graph.replay()
    graph.synchronize()
    got = out.to_numpy().copy()
    eager = moe(dev(x2)).to_numpy()
    np.testing.assert_array_equal(got, eager)
    assert rel_err(O.bf16_bits_to_f32(got), ref(x2)) < 1e-2


# ----------------------------------------------------------------------------------------------------- end to end
TINY = dict(vocab_size=512, hidden_size=256, num_layers=4, num_heads=4, num_kv_heads=2, head_dim=64, intermediate_size=128,
            rope_theta=1e6, norm_eps=1e-6)


def _bf16(x):
    return O.f32_to_bf16_bits(np.ascontiguousarray(x, np.float32))


def tiny_moe_weights(seed, E=8):
    """Qwen3-style weights plus a router and experts per layer.  Dims 0..7 of every token's embedding hold a distinct
    permutation of 0.25, 0.5, ..., 2.0, no projection writes them, and the router reads them: each token has its own,
    clearly separated routing (a random router over random hidden states leaves near-ties that bf16 activations would
    flip).  The untied lm_head leaves those dims out, so they do not decide the next token."""
    w = O.make_qwen3_weights(TINY, seed=seed, bf16=True)
    rng = np.random.default_rng(seed + 100)
    perms = set()
    while len(perms) < TINY["vocab_size"]:
        perms.add(tuple(rng.permutation(E)))
    w["embed"][:, :E] = (np.array(sorted(perms, key=lambda _: rng.random()), np.float32) + 1) * np.float32(0.25)
    w["lm_head"] = w["embed"].copy()
    w["lm_head"][:, :E] = 0.0
    for lw in w["layers"]:
        lw["o"][:E] = 0.0
        router = rng.standard_normal((E, TINY["hidden_size"])).astype(np.float32) * np.float32(0.002)
        router[:, :E] += np.float32(0.5) * np.eye(E, dtype=np.float32)
        lw["router"] = O.bf16_round(router)
        lw["experts"] = [tuple(O.bf16_round(rng.standard_normal(s).astype(np.float32) * np.float32(std))
                               for s, std in (((128, 256), 0.05), ((128, 256), 0.05), ((256, 128), 0.02))) for _ in range(E)]
        for _, _, d in lw["experts"]:
            d[:E] = 0.0
    return w


def write_checkpoint(tmp_path, w, family, fp8=False, E=8, k=2):
    t = {"model.embed_tokens.weight": (_bf16(w["embed"]), "BF16"), "model.norm.weight": (_bf16(w["final_norm"]), "BF16"),
         "lm_head.weight": (_bf16(w["lm_head"]), "BF16")}
    moe = "block_sparse_moe" if family == "mixtral" else "mlp"
    names = ("w1", "w3", "w2") if family == "mixtral" else ("gate_proj", "up_proj", "down_proj")
    for i, lw in enumerate(w["layers"]):
        L = f"model.layers.{i}."
        t[L + "input_layernorm.weight"] = (_bf16(lw["attn_norm"]), "BF16")
        t[L + "post_attention_layernorm.weight"] = (_bf16(lw["mlp_norm"]), "BF16")
        if family == "qwen3_moe":
            t[L + "self_attn.q_norm.weight"] = (_bf16(lw["q_norm"]), "BF16")
            t[L + "self_attn.k_norm.weight"] = (_bf16(lw["k_norm"]), "BF16")
        for key, name in (("q", "q_proj"), ("k", "k_proj"), ("v", "v_proj"), ("o", "o_proj")):
            t[L + f"self_attn.{name}.weight"] = (_bf16(lw[key]), "BF16")
        t[L + f"{moe}.gate.weight"] = (_bf16(lw["router"]), "BF16")
        for e, ex in enumerate(lw["experts"]):
            for m, nm in zip(ex, names):
                base = L + f"{moe}.experts.{e}.{nm}.weight"
                if fp8:
                    codes, sbits = O.quantize_fp8_e4m3_block(m)
                    t[base] = (codes, "F8_E4M3")
                    t[base + "_scale_inv"] = (sbits, "BF16")
                else:
                    t[base] = (_bf16(m), "BF16")
    p = str(tmp_path / "model.safetensors")
    ST.save_safetensors(p, t, {"format": "pt"})
    conf = {"model_type": family, "rope_theta": TINY["rope_theta"], "rms_norm_eps": TINY["norm_eps"],
            "max_position_embeddings": 256, "num_experts_per_tok": k}
    if family == "mixtral":
        conf.update(num_local_experts=E, intermediate_size=128)
    else:
        conf.update(num_experts=E, moe_intermediate_size=128, intermediate_size=768, norm_topk_prob=True,
                    decoder_sparse_step=1, mlp_only_layers=[])
    if fp8:
        conf["quantization_config"] = {"quant_method": "fp8", "fmt": "e4m3", "weight_block_size": [128, 128]}
    (tmp_path / "config.json").write_text(json.dumps(conf))
    return p


def ref_model(w, family, fp8, k=2):
    ref = O.build_qwen3_ref(TINY, w if family == "qwen3_moe" else dict(w, layers=[{kk: v for kk, v in lw.items() if kk not in (
        "q_norm", "k_norm")} for lw in w["layers"]]), max_pos=256)
    ref._lm_head = w["lm_head"]
    moes = []
    for blk, lw in zip(ref.blocks, w["layers"]):
        ex = lw["experts"]
        if fp8:
            ex = [tuple(O.dequantize_fp8_e4m3_block(*O.quantize_fp8_e4m3_block(m)) for m in e) for e in ex]
        blk.mlp = R.RefMoE(lw["router"], ex, k)
        moes.append(blk.mlp)
    return ref, moes


@pytest.mark.parametrize("family, fp8", [("qwen3_moe", False), ("mixtral", False), ("qwen3_moe", True)])
def test_tiny_moe_checkpoint_end_to_end(tmp_path, family, fp8):
    from pygpukit_amd.llm.loader import load_model_from_safetensors

    prompt = [int(t) for t in np.random.default_rng(6).integers(0, TINY["vocab_size"], 12)]
    # pick weights whose oracle routing (prefill and the greedy steps) keeps every top-k margin clear of rounding
    for seed in range(40, 80):
        w = tiny_moe_weights(seed)
        ref, moes = ref_model(w, family, fp8)
        want_tokens = ref.generate(prompt, max_new_tokens=4, temperature=0.0, top_k=0, top_p=1.0)
        if min(m.min_margin for m in moes) > 0.03:
            break
    else:
        pytest.fail("no seed with clear routing margins")
    model = load_model_from_safetensors(write_checkpoint(tmp_path, w, family, fp8))
    c = model.config
    assert model.spec.name == family and c.is_moe and (c.num_experts, c.num_experts_per_tok, c.moe_intermediate_size) == (8, 2, 128)
    assert isinstance(model.blocks[0].mlp, MoELayer) and model.blocks[0].mlp.fp8 == fp8
    hid, _ = ref(prompt)
    h, _ = model(prompt)
    assert rel_err(O.bf16_bits_to_f32(model.get_logits(h).to_numpy()), ref.get_logits(hid)) < 1e-2
    assert model.generate(prompt, max_new_tokens=4, temperature=0.0, top_k=0, top_p=1.0) == want_tokens
    with pytest.raises(NotImplementedError, match="the native engine covers dense models"):
        model.build_engine()
