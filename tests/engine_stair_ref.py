"""A probe model whose logits read out which key the native engine's attention saw (NumPy only).

tests/attn_stair_ref.py builds Q / K / V so that an attention OP returns the V row of its highest visible key.  The engine
takes token ids, not tensors, so here the WEIGHTS of a one-layer model do the same through the unmodified engine
(hidden_size == num_heads * head_dim):

    token id = tag * 4096 + height          height 0 .. 4095, tag 0 .. 3 (the sequence slot), vocabulary 16384
    embedding row x: dimension 0 holds 1, dimensions 1 .. 12 the height's bits, 13 .. 24 their complements, 25 .. 28 the
        one-hot tag, every other dimension +-1 fixed per token id -> every row has H - 15 ones: RMSNorm multiplies every
        row by ONE factor c, and the normalised row is c * x with x in {0, +-1} (its bf16 rounding is one factor too)
    K: column HALF-12+b of every kv head copies bit b, column D-12+b (its rotate-half partner) the complement, every
        other column copies one +-1 noise dimension (each weight row has a single non-zero entry): every K row has
        12 + (D - 24) entries of magnitude c - one norm, so QK-norm multiplies every row by one factor as well.  The 24
        columns sit at the lowest RoPE frequencies and rope_theta = 1e30: cos rounds to 1.0f and the partner's share
        other * sin is below 1e-15 of it (check_rope)
    Q: column HALF-12+b = s * 2**b read from dimension 0 - powers of two, one significand, so 1/sqrt(D), the RMS factors,
        the QK-norm scale and the bf16 rounding of q scale the whole staircase by one factor; every other column
        N(0,1)/8 noise.  With QK-norm on the norm divides s out again and the amplifier is q_norm's gamma on those columns
    -> score(key j) = step * height(j) + noise, step >= MIN_STEP = 60 natural-log units (staircase_step)
    V = W_v . x with random W_v: rows differ per token, per slot (tag and noise dimensions) and per kv head
    W_o = identity, W_down = 0 (gate / up random, so those kernels run on real data), final norm gamma 1,
    lm_head = identity on its first H rows, zero elsewhere (passed to Engine(...) explicitly)
    -> logits[:H] = rmsnorm(x[token] + V_row),   V_row = the cache row of the highest visible height, per kv head,
       repeated over its query heads;  logits[H:] = 0

The probability of the winning key is exactly 1.0 and every other weight is below exp(-60) < 2**-86, W_o contributes one
non-zero product per output, so NOTHING is counted for attention and o_proj: the bar (logit_bar) is fp32 RMSNorm over H
terms and the fp32 store, plus one bf16 rounding (BF16_U = 2**-8) where the path's lm_head reads bf16 activations.
"""

from __future__ import annotations

import functools
import math

import numpy as np

from oracle import cpu_ref as O

F32, F64 = np.float32, np.float64
VOCAB, NBITS, NTAGS = 16384, 12, 4
TOP = 4095                      # the height a one-token prefill plants in the middle of a context (contexts <= 4094: rows below 4094)
FILL_MAX = 4095                 # ascending fill: row j holds height min(j + 1, FILL_MAX), always above a height-0 query token
MIN_STEP = 60.0
# One round-to-nearest bf16 store: 8 significant bits, so half a unit in the last place is 2**-8 of the binade's lower end -
# the format's unit roundoff.  (Half of it, 2**-9, is missed by a correctly rounded value just above a power of two, and by
# the fp32 emulation of tests/test_engine_stair_cpu.py.)
BF16_U = 2.0 ** -8
PRECONDITION = 2.0 ** -20
ROPE_THETA = 1e30
EPS = 1e-6
INTERMEDIATE = 256
DIM_ONE, DIM_BIT0, DIM_CMP0, DIM_TAG0, DIM_NOISE0 = 0, 1, 1 + NBITS, 1 + 2 * NBITS, 1 + 2 * NBITS + NTAGS

# name -> (head_dim, query heads per kv head, kv heads)
SHAPES = {"d128g1": (128, 1, 2), "d128g2": (128, 2, 2), "d128g4": (128, 4, 1), "d64g2": (64, 2, 2), "d128g7": (128, 7, 1)}


def token(height, tag=0):
    return np.asarray(tag, np.int64) * 4096 + np.asarray(height, np.int64)


def fill_heights(n: int) -> np.ndarray:
    return np.minimum(np.arange(n) + 1, FILL_MAX)


def fill_tokens(n: int, tag: int = 0) -> list[int]:
    """Ascending heights for cache rows 0 .. n-1 of slot `tag`."""
    return [int(t) for t in token(fill_heights(n), tag)]


def encode_e4m3_blocks(w: np.ndarray):
    """w [N, K] (N, K multiples of 128) -> (e4m3 codes uint8 [N, K], bf16 words of the block scales [N/128, K/128], the
    dequantised matrix): per 128 x 128 block the scale is the POWER OF TWO that puts the block's largest entry into
    (224, 448], codes round to nearest even.  Powers of two within 2**-11 of the block's largest entry, +-1 and 0 are exact."""
    N, K = w.shape
    assert N % 128 == 0 and K % 128 == 0
    blocks = w.astype(F64).reshape(N // 128, 128, K // 128, 128)
    absmax = np.abs(blocks).max(axis=(1, 3))
    exps = np.where(absmax > 0, np.ceil(np.log2(np.where(absmax > 0, absmax, 1.0) / 448.0)), 0.0)
    scale = (2.0 ** exps)[:, None, :, None]
    codes = O._rne_e4m3_codes((blocks / scale).astype(F32)).reshape(N, K)
    deq = (O.fp8_e4m3_table()[codes].astype(F64).reshape(blocks.shape) * scale).reshape(N, K).astype(F32)
    sbits = O.f32_to_bf16_bits((2.0 ** exps).astype(F32))
    assert np.array_equal(O.bf16_bits_to_f32(sbits), (2.0 ** exps).astype(F32)) and np.isfinite(deq).all()
    return codes, sbits, deq


class Probe:
    """Config, fp32 (bf16-exact) weights in the oracle's layout (+ "lm_head"), and the closed forms the tests need."""

    def __init__(self, shape: str, qk_norm: bool, fp8: bool = False):
        D, G, Hkv = SHAPES[shape]
        self.is_fp8 = fp8
        Hq, H, HALF = G * Hkv, G * Hkv * D, D // 2
        self.shape, self.qk_norm, self.D, self.G, self.Hkv, self.Hq, self.H = shape, qk_norm, D, G, Hkv, Hq, H
        self.cfg = dict(vocab_size=VOCAB, hidden_size=H, num_layers=1, num_heads=Hq, num_kv_heads=Hkv, head_dim=D,
                        intermediate_size=INTERMEDIATE, rope_theta=ROPE_THETA, norm_eps=EPS)
        rng = np.random.default_rng(1000 * D + 10 * G + Hkv + (5 if qk_norm else 0))
        self.bit_cols = HALF - NBITS + np.arange(NBITS)          # lowest RoPE frequencies: the pairs nearest D/2
        self.cmp_cols = D - NBITS + np.arange(NBITS)
        info = np.concatenate([self.bit_cols, self.cmp_cols])
        self.noise_cols = np.setdiff1d(np.arange(D), info)
        # ---- embedding
        ids = np.arange(VOCAB)
        emb = rng.choice(np.array([-1.0, 1.0], F32), size=(VOCAB, H))
        emb[:, DIM_ONE] = 1.0
        bits = ((ids[:, None] % 4096) >> np.arange(NBITS)[None, :]) & 1
        emb[:, DIM_BIT0:DIM_BIT0 + NBITS] = bits
        emb[:, DIM_CMP0:DIM_CMP0 + NBITS] = 1 - bits
        emb[:, DIM_TAG0:DIM_TAG0 + NTAGS] = np.eye(NTAGS, dtype=F32)[ids // 4096]
        assert np.all((emb.astype(F64) ** 2).sum(1) == H - 15)
        self.c = 1.0 / math.sqrt((H - 15) / H + EPS)             # RMSNorm's factor, the same for every token
        # ---- K
        wk = np.zeros((Hkv * D, H), F32)
        for kh in range(Hkv):
            r0 = kh * D
            wk[r0 + self.bit_cols, DIM_BIT0 + np.arange(NBITS)] = 1.0
            wk[r0 + self.cmp_cols, DIM_CMP0 + np.arange(NBITS)] = 1.0
            src = rng.choice(np.arange(DIM_NOISE0, H), size=self.noise_cols.size, replace=False)
            wk[r0 + self.noise_cols, src] = rng.choice(np.array([-1.0, 1.0], F32), size=src.size)
        assert np.all((wk != 0).sum(1) == 1)
        k_rms = math.sqrt(self.c ** 2 * (D - NBITS) / D + EPS)
        self.kappa = self.c / k_rms if qk_norm else self.c        # a set bit's value in the K cache, before bf16
        # ---- Q
        wq = O.bf16_round(rng.standard_normal((Hq * D, H)).astype(F32) / F32(8.0 * math.sqrt(H)))
        q_gamma = np.ones(D, F32)
        scale = 1.0 / math.sqrt(D)
        lo = 1.0 - 2.0 ** -6                                      # room for the bf16 roundings of c, q and k
        if qk_norm:
            s = 1.0
            q_rms_hi = math.sqrt((self.c ** 2 * (4.0 ** NBITS) / 3.0 + D) / D)   # stair columns + a generous bound on the noise columns
            unit = self.c / q_rms_hi * self.kappa * scale * lo    # step per unit of gamma
            g = 1.0
            while g * unit < MIN_STEP:
                g *= 2.0
            q_gamma[self.bit_cols] = g
            self.amplifier = g
        else:
            unit = self.c * self.c * scale * lo
            s = 1.0
            while s * unit < MIN_STEP:
                s *= 2.0
            self.amplifier = s
        for h in range(Hq):
            wq[h * D + self.bit_cols, :] = 0.0
            wq[h * D + self.bit_cols, DIM_ONE] = s * 2.0 ** np.arange(NBITS)
        assert np.array_equal(O.bf16_round(wq), wq) and np.array_equal(O.bf16_round(q_gamma), q_gamma)
        self.step_lo = self.amplifier * unit
        assert self.step_lo >= MIN_STEP
        # ---- V, readout, MLP
        wv = O.bf16_round((rng.standard_normal((Hkv * D, H)) * 0.05).astype(F32))
        I = INTERMEDIATE
        layer = dict(q=wq, k=wk, v=wv, o=np.eye(H, dtype=F32), gate=O.bf16_round((rng.standard_normal((I, H)) * 0.02).astype(F32)),
                     up=O.bf16_round((rng.standard_normal((I, H)) * 0.02).astype(F32)), down=np.zeros((H, I), F32),
                     attn_norm=np.ones(H, F32), mlp_norm=np.ones(H, F32))
        if qk_norm:
            layer.update(q_norm=q_gamma, k_norm=np.ones(D, F32))
        self.fp8 = None
        if fp8:
            # w8a16: every linear as e4m3 codes under power-of-two 128 x 128 block scales, encoded HERE (encode_e4m3_blocks) and
            # handed to the engine as they are.  The model is the DEQUANTISED weights: the stair, the copying W_k and the
            # identity W_o are exact, the random matrices move to the e4m3 grid, Q noise next to the stair may flush to zero.
            fused = {"w_qkv": np.concatenate([wq, wk, wv]), "w_o": layer["o"], "w_gate_up": np.concatenate([layer["gate"], layer["up"]]),
                     "w_down": layer["down"]}
            self.fp8, deq = {}, {}
            for name, m in fused.items():
                codes, sbits, deq[name] = encode_e4m3_blocks(m)
                self.fp8[name] = (codes, sbits)
            nq, nk = Hq * D, Hkv * D
            dq, dk, wv = deq["w_qkv"][:nq], deq["w_qkv"][nq:nq + nk], deq["w_qkv"][nq + nk:]
            for h in range(Hq):
                assert np.array_equal(dq[h * D + self.bit_cols], wq[h * D + self.bit_cols]), "the stair is not exact in e4m3"
            assert np.array_equal(dk, wk) and np.array_equal(deq["w_o"], layer["o"]) and not deq["w_down"].any()
            layer.update(q=dq, k=dk, v=wv, o=deq["w_o"], gate=deq["w_gate_up"][:I], up=deq["w_gate_up"][I:], down=deq["w_down"])
            for a in deq.values():
                assert np.array_equal(O.bf16_round(a), a)          # what the MFMA paths round to bf16 is what the GEMVs multiply
        lm = np.zeros((VOCAB, H), F32)
        lm[:H] = np.eye(H, dtype=F32)
        self.weights = {"embed": emb, "layers": [layer], "final_norm": np.ones(H, F32), "lm_head": lm}
        for a in (emb, lm, *[v for v in layer.values()]):
            a.setflags(write=False)
        self.wv_abs = np.abs(wv.astype(F64)).sum(1) * self.c      # sum_j |w_j * c x_j|: x is +-1 or 0 (a bound; 15 entries are 0)

    # ---- closed forms -------------------------------------------------------------------------------------------------
    def x(self, toks) -> np.ndarray:
        return self.weights["embed"][np.asarray(toks, np.int64)].astype(F64)

    def v_rows(self, toks) -> np.ndarray:
        """float64 W_v . rmsnorm(x): [n, Hkv, D]."""
        v = (self.x(toks) * self.c) @ self.weights["layers"][0]["v"].astype(F64).T
        return v.reshape(len(v), self.Hkv, self.D)

    def v_bar(self, v64: np.ndarray) -> np.ndarray:
        """Bound on |cache V - v64| per element [.., Hkv, D]: the normalised row's common bf16 rounding (paths with bf16
        activations) and the row's own bf16 rounding, BF16_U each, plus fp32 accumulation of H products."""
        return np.abs(v64) * ((1.0 + BF16_U) ** 2 - 1.0) + (self.H + 4) * 2.0 ** -24 * self.wv_abs.reshape(self.Hkv, self.D)

    def k_bit_word(self) -> int:
        """The bf16 word of a set bit (or set complement) in the K cache."""
        return int(O.f32_to_bf16_bits(np.array([self.kappa], F32))[0])

    def k_zero_bound(self, max_pos: int) -> float:
        """A cleared bit holds -+kappa * sin(angle) of its partner: below this."""
        return 2.0 * self.kappa * max_pos * ROPE_THETA ** (-2.0 * float(self.bit_cols[0]) / self.D)

    def k_expected_bits(self, toks) -> np.ndarray:
        """[n, 24] 0/1: what the bit columns then the complement columns of every kv head hold for these tokens."""
        h = np.asarray(toks, np.int64) % 4096
        bits = (h[:, None] >> np.arange(NBITS)[None, :]) & 1
        return np.concatenate([bits, 1 - bits], axis=1)

    def logits_from_v(self, tok: int, v_row: np.ndarray) -> np.ndarray:
        """float64 logits[:H] of the readout for query token `tok` and attention output V row [Hkv, D] (as read from the cache)."""
        o = np.repeat(np.asarray(v_row, F64), self.G, axis=0).reshape(self.H)     # query head h reads kv head h // G
        h = self.x([tok])[0] + o
        return h / np.sqrt(np.mean(h * h) + EPS)

    def logit_bar(self, want: np.ndarray, n_bf16: int) -> np.ndarray:
        """Per-element bound on |logits - want|: h = x + o (1 rounding), H squares and their sum (H/2 after the square
        root), mean, + eps, rsqrt, two products and the store (8 in all), then n_bf16 bf16 roundings of BF16_U."""
        rel = (1.0 + (self.H / 2 + 8) * 2.0 ** -24) * (1.0 + BF16_U) ** n_bf16 - 1.0
        return rel * np.abs(want) + 1e-30

    # ---- preconditions ----------------------------------------------------------------------------------------------
    def check_rope(self, max_pos: int) -> None:
        """cos of every stair column rounds to 1.0f and |other * sin| is below half an ulp, at every position of the cache."""
        i = float(self.bit_cols[0])                               # the highest of the stair frequencies
        ang = (max_pos - 1) * ROPE_THETA ** (-2.0 * i / self.D)
        assert F32(math.cos(ang)) == F32(1.0), (self.shape, ang)
        assert abs(math.sin(ang)) < 2.0 ** -25, (self.shape, ang)
        # cleared bits add nothing to a score: all stair weights together are below 2 * step * 2**NBITS per unit of kappa
        assert 2.0 * self.step_lo * 2.0 ** NBITS * self.k_zero_bound(max_pos) / self.kappa < 2.0 ** -20

    def check_k_word(self) -> None:
        """kappa is at least 2**-6 of a bf16 ulp (2**-14 relative) away from a rounding tie.  fp32 arithmetic in any order
        (RMSNorm over H or D terms: at most (H/2 + 8) * 2**-24 < 2**-15 relative for H <= 896) then gives one word."""
        m, _ = math.frexp(self.kappa)
        frac = (m * 256.0) % 1.0
        assert (self.H / 2 + 8) * 2.0 ** -24 < 2.0 ** -15
        assert abs(frac - 0.5) > 2.0 ** -6, (self.shape, self.kappa)


@functools.lru_cache(maxsize=None)
def probe(shape: str, qk_norm: bool = True, fp8: bool = False) -> Probe:
    return Probe(shape, qk_norm, fp8)


# ---- the fp64 oracle on the probe (or any) weights ---------------------------------------------------------------------------

def oracle_model(cfg: dict, weights: dict, max_pos: int):
    w64 = {"embed": weights["embed"].astype(F64), "final_norm": weights["final_norm"].astype(F64),
           "layers": [{k: v.astype(F64) for k, v in lw.items()} for lw in weights["layers"]]}
    if "lm_head" in weights:
        w64["lm_head"] = weights["lm_head"].astype(F64)
    return O.build_qwen3_ref(cfg, w64, max_pos=max_pos)


def oracle_cache(ref, toks, chunk: int = 512, start: int = 0):
    """Per layer (k, v) [n, Hkv, D] of the oracle after a chunked prefill of `toks` at positions start .. (fp64).  A
    ONE-layer model's K / V rows depend on the token and its position only, so its chunks run without the rows before them."""
    if len(ref.blocks) == 1:
        parts = [ref(list(toks[i:i + 128]), position_ids=list(range(start + i, start + min(i + 128, len(toks)))), use_cache=True)[1][0]
                 for i in range(0, len(toks), 128)]
        return [(np.concatenate([k for k, _ in parts]), np.concatenate([v for _, v in parts]))]
    assert start == 0
    past = None
    for i in range(0, len(toks), chunk):
        _, past = ref(list(toks[i:i + chunk]), past_key_values=past, use_cache=True)
    return past


def oracle_step(ref, past, tok: int, pos: int, rows=None) -> np.ndarray:
    """Logits of query token `tok` at position `pos` that sees the cache rows `rows` (default: 0 .. pos-1, the causal
    mask) and itself.  Rows carry their RoPE position, so any subset is a mutated MASK, not a moved key."""
    rows = np.arange(pos) if rows is None else np.asarray(rows, np.int64)
    sub = [(k[rows], v[rows]) for k, v in past]
    hidden, _ = ref([int(tok)], position_ids=[int(pos)], past_key_values=sub, use_cache=True)
    return np.asarray(ref.get_logits(hidden))[0]


def nearest_row(p: Probe, tok: int, got: np.ndarray, v_cache: np.ndarray, kvh: int = 0):
    """Which cache row's V the returned logits are nearest to, for kv head `kvh`: v_cache [slots, Hkv, rows, D] (float),
    got [H].  Returns (slot, kv head, row, distance).  Every (slot, kv head, row) is a candidate: a wrong slot or kv head
    shows as such."""
    blk = slice(kvh * p.G * p.D, kvh * p.G * p.D + p.D)          # the first query head of that kv head
    x = p.x([tok])[0][blk]
    g = np.asarray(got, F64)[blk]
    # logits = (x + v) * r with one unknown positive factor r: compare directions
    cand = x[None, None, None, :] + np.asarray(v_cache, F64)
    cand /= np.linalg.norm(cand, axis=-1, keepdims=True) + 1e-300
    d = np.linalg.norm(cand - g / (np.linalg.norm(g) + 1e-300), axis=-1)
    s, h, r = np.unravel_index(int(np.argmin(d)), d.shape)
    return int(s), int(h), int(r), float(d[s, h, r])


# ---- contexts, shared by the CPU precondition tests and the GPU tests ------------------------------------------------------
CACHE_SHORT, CACHE_LONG = 512, 4096
# the fused batch-1 kernels: tile edges (16), pair edges (64), the staging edge (128), the 192-row chunk / preload,
# 256 / 320 (trips of 128 behind the preload), the last fused positions 383 and the first split one 384
FUSED_CTX = (0, 1, 15, 16, 17, 63, 64, 127, 128, 129, 143, 144, 145, 159, 160, 176, 190, 191, 192, 193, 208, 256, 320, 383)
SPLIT_CTX = (385, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4094, 4095)
SPLIT_SHORT_CTX = (1, 63, 64, 65, 191, 192, 193, 383, 384)      # PGK_FUSED_ATTN=0: the split-KV sequence at short contexts
# dealt to the sequences of a batch, moved on by one for every 16 sequences (test_engine_stair_gpu.batch_positions), so that no two
# sequences of a batch share both their tag and their position
BATCH_CTX = (191, 192, 193, 383, 384, 511, 510, 1, 16, 129, 255, 256, 320, 448, 500, 64)
ALL_CTX = tuple(sorted(set(FUSED_CTX + SPLIT_CTX + SPLIT_SHORT_CTX + BATCH_CTX + (100, 513, 600, 1000, 2000))))
PLANT_CTX = (129, 192, 193, 320, 383)                             # short contexts at which a top height is planted in every position group
# (shape, QK-norm): Qwen3 family (on) for every shape, Llama family (off) for the two shapes that reach every kernel
FP8_PROBES = [("d128g2", True), ("d128g2", False), ("d64g2", True)]     # w8a16 engines
PROBES = [("d128g1", True), ("d128g2", True), ("d128g2", False), ("d128g4", True), ("d64g2", True), ("d64g2", False), ("d128g7", True)]


def plant_rows_short(pos: int, D: int) -> list[int]:
    """One row per position group of the context [0, pos) (16 rows at head_dim 128, 32 at 64), at a varying offset."""
    grp = 4 * (64 // (D // 8))
    rows = [g + (7 * (g // grp)) % grp for g in range(0, pos, grp)]
    return [m for m in rows if m < pos]


def slice_edge_rows(pos: int, span: int, nsplit: int, D: int) -> list[int]:
    """First and last row of every split-KV slice that holds cached rows of the context [0, pos): slices are cut by
    absolute position, `nsplit` of them over `span` rows in whole position-group steps (decode_chunk_len)."""
    grp = 4 * (64 // (D // 8))
    chunk = max(grp, -(-(-(-span // nsplit)) // grp) * grp)
    rows = set()
    for c0 in range(0, pos, chunk):
        rows.update((c0, min(c0 + chunk, pos) - 1))
    return sorted(rows)


PREFILL_LENS = (1, 15, 16, 17, 127, 128, 129, 255, 256, 257, 1000)
PREFILL_CHUNKS = (5, 1, 3, 120)                                   # then the rest


def prefill_prompt(n: int, kind: str, tag: int = 0):
    """(tokens, winner): `winner[i]` is the row whose V row i must return.  "ascending": heights 1 .. n, every row returns
    itself.  "descending": five ascending rows on top (heights n+1 .. n+5), then n, n-1, ...: every later row returns
    row 4, the top of the first chunk."""
    i = np.arange(n)
    if kind == "ascending":
        return [int(t) for t in token(i + 1, tag)], i
    n0 = min(PREFILL_CHUNKS[0], n)
    heights = np.where(i < n0, n + 1 + i, n - (i - n0))
    assert heights.min() >= 1 and heights.max() <= 4095
    return [int(t) for t in token(heights, tag)], np.where(i < n0, i, n0 - 1)


def prefill_chunks(n: int) -> list[tuple[int, int]]:
    """(start, length) of the ragged chunks 5 + 1 + 3 + 120 + the rest."""
    out, start = [], 0
    for c in PREFILL_CHUNKS:
        if start >= n:
            break
        out.append((start, min(c, n - start)))
        start += out[-1][1]
    if start < n:
        out.append((start, n - start))
    return out
