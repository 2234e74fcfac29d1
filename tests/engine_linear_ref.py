"""Probe models whose readouts are exact per-element functions of ONE projection of the native engine (NumPy only).

The engine's five projections (w_qkv, w_o, w_gate_up, w_down, lm_head) are checked through whole-model logits elsewhere.
Here one-layer models (plus a two-layer variant whose first layer passes the residual stream through) make every output
element of one "live" projection readable through the unmodified engine - prefill, set_state, decode_step, capture / replay,
logits, all_logits, kv_cache, read_tokens - while every other projection is an exact pass-through.

The arithmetic is exact by construction:

    embedding        every entry +-1 (dimension 0: +1 in every row, dimensions 1 .. 12: the token id's bits as +-1), so the
                     mean square is exactly 1 and RMSNorm's factor is c = 1 / sqrt(1 + eps) for every token: 0.9999995 in
                     fp32, exactly 1.0 after a bf16 rounding (check_constants)
    norm gammas      +-1 and +-2, fixed per column, drawn with unequal weights (a gamma indexing error changes values)
    live matrices    -1, 0, +1 (times one power of two): exact as bf16 rows, as e4m3 codes under power-of-two 128 x 128 block
                     scales and as NVF4 codes under power-of-two scale bytes.  The probe encodes fp8 and NVF4 itself (the
                     project's quantisers are not used); neighbouring scale blocks get DIFFERENT (scale, code) pairs for
                     the same value - exponent +1 on odd blocks - so a scale taken from the neighbouring block changes values
    rope_theta       2**64: every RoPE frequency is a power of two in any powf, the angle of the first pair is the position

so a projection that reads bf16 activations returns integer sums of at most K terms - exact in fp32 in any order and exact
again after a bf16 store while |sum| <= 256 - and one that reads fp32 activations (GEMV chunks of 1 and 2 sequences)
returns c32 x integer inside a derived accumulation bar.

Probes (kind):
    "QL"   w_qkv and lm_head live (dense +-1); w_o = w_gate_up = w_down = 0.  K and V rows are read from the cache (V and K
           at position 0 bit for bit, K at later positions against the oracle's RoPE); logits = lm_head . norm(x) are V
           integers; the next token is the oracle's lowest-index argmax, with one exact duplicate of one token's winning
           row planted 2048 rows away.  Every K and V sum is odd (see Probe).
    "O"    w_o live; W_v a signed selection, w_down = 0, lm_head = identity on its first H rows:
           logits[:H] = rmsnorm(x + W_o . v).  Decode runs at position 0 (one visible key: the V row comes back unchanged);
           prefill uses own-row attention by a +-1 staircase (Q columns s * 2**b read dimension 0, K columns copy the +-1
           id bits: score = step * (2 id - 4095), ascending ids, so row t returns its own V row with probability exactly 1.0).
    "GUa"  gate live and sparse (g = 64 + sum in [17, 256]: silu(g) = g in fp32), up a signed +-1 / +-2 selection,
    "GUb"  up live, gate = 32 or 64 from dimension 0;  both: w_down a selection x 2**-5 of the H-wide slice `sl` of I
           (one engine per slice), logits[:H] = rmsnorm(x + act slice / 32).  act_n = g_n * u_n: a gate row paired with the
           wrong up row changes it.
    "D"    w_down live with entries +-2**-5; gate 32 from dimension 0, up a signed selection: act = +-32, +-64.

Out of reach, on purpose: the Q rows of w_qkv land nowhere readable (only K and V are stored; Q stays covered by the
whole-step tests and, on the O probe, by the staircase it has to produce); the NVF4 prefill o_proj probe (the staircase's
twelve powers of two do not fit one NVF4 scale block - the NVF4 O probe has no staircase and is decoded at position 0
only); GU on fp8a8 (the integer act is not representable in e4m3).
"""

from __future__ import annotations

import functools
import math

import numpy as np

from oracle import cpu_ref as O
from tests import engine_stair_ref as ST
from tests import nvf4_engine_ref as NV

F32, F64 = np.float32, np.float64
EPS = 1e-6
C64 = 1.0 / math.sqrt(1.0 + EPS)
C32 = float(F32(1.0) / np.sqrt(F32(1.0) + F32(EPS)))
THETA = 2.0 ** 64
NBITS = 12
VOCAB = 4096
DUP_TOKEN, DUP_SHIFT = 7, 2048
U24 = 2.0 ** -24
BF16_U = ST.BF16_U
MIN_STEP = ST.MIN_STEP

# H, I, query heads, kv heads, head_dim.  W: the benchmark's widths (qkv N = 4096: 4 rows per wave at K = 1024; gate_up 6 rows
# per wave; down at K = 3072).  W6: 2176 pairs leave 6-row workgroups a tail.  T: generic K everywhere, head_dim 64, GQA 3.
# X: K = 512 and 1536 (preload depths 1 and 3), qkv N = 2048 (2 rows per wave).  P: K = 256 in o_proj - no carried norms, so
# the packed decode step keeps its split-K slabs.  B4: 4096 gate / up pairs (4 pair rows per wave); down at K = 4096 (the
# register-fragment batched kernel's deepest width, 32 k-steps per wave).
SHAPES = {"W": (1024, 3072, 16, 8, 128), "W6": (1024, 2176, 16, 8, 128), "T": (640, 896, 6, 2, 64), "X": (512, 1536, 8, 4, 128),
          "P": (512, 1024, 2, 1, 128), "B4": (512, 4096, 4, 2, 128)}
DENSITY = {"QL": 0.35, "LM": 0.35, "O": 0.3, "GUb": 0.35, "D": 0.25}
GATE_NNZ = 40


def check_constants() -> None:
    assert C32 == float(F32(0.9999995)) and O.bf16_round(np.array([C32], F32))[0] == 1.0
    m = np.arange(-256, 257).astype(F32)
    assert np.array_equal(O.bf16_round(m * F32(C32)), m)          # bf16(c32 * m) = m for |m| <= 256


def sparse_pm1(rng, n: int, k: int, density: float) -> np.ndarray:
    w = rng.choice(np.array([-1.0, 1.0], F32), size=(n, k))
    w[rng.random((n, k)) >= density] = 0.0
    return w


def gammas(rng, n: int) -> np.ndarray:
    return rng.choice(np.array([1.0, -1.0, 2.0, -2.0], F32), size=n, p=[0.4, 0.3, 0.2, 0.1])


def selection(n_rows: int, k: int, mult: int, off: int, mags=(1.0,)) -> np.ndarray:
    """Row n holds one entry at column (n * mult + off) % k: sign and magnitude vary with n in fixed, unequal patterns."""
    w = np.zeros((n_rows, k), F32)
    n = np.arange(n_rows)
    sign = np.where((n * 5 + n // 7) % 3 == 0, -1.0, 1.0)
    mag = np.asarray(mags, F32)[(n + n // 5) % len(mags)]
    w[n, (n * mult + off) % k] = sign * mag
    return w


# ---- hand encoders ------------------------------------------------------------------------------------------------------------

def encode_fp8(w: np.ndarray):
    """[N, K] -> (e4m3 codes, bf16 words of the 128 x 128 block scales): power-of-two scales, the block's largest entry in
    (112, 448] - one exponent higher on blocks with odd (row block + column block), so neighbours differ.  Exact or an error."""
    N, K = w.shape
    assert N % 128 == 0 and K % 128 == 0
    blocks = w.astype(F64).reshape(N // 128, 128, K // 128, 128)
    absmax = np.abs(blocks).max(axis=(1, 3))
    amax_all = float(np.abs(w).max()) or 1.0
    absmax = np.where(absmax > 0, absmax, amax_all)                # an all-zero block takes the matrix's scale
    odd = (np.arange(N // 128)[:, None] + np.arange(K // 128)[None, :]) % 2
    exps = np.ceil(np.log2(absmax / 448.0)) + odd
    scale = (2.0 ** exps)[:, None, :, None]
    codes = O._rne_e4m3_codes((blocks / scale).astype(F32)).reshape(N, K)
    deq = (O.fp8_e4m3_table()[codes].astype(F64).reshape(blocks.shape) * scale).reshape(N, K)
    assert np.array_equal(deq, w.astype(F64)), "not exact in e4m3 under power-of-two block scales"
    sbits = O.f32_to_bf16_bits((2.0 ** exps).astype(F32))
    assert np.array_equal(O.bf16_bits_to_f32(sbits).astype(F64), 2.0 ** exps)
    return codes, sbits


def decode_fp8(codes: np.ndarray, sbits: np.ndarray) -> np.ndarray:
    s = np.repeat(np.repeat(O.bf16_bits_to_f32(sbits).astype(F64), 128, 0), 128, 1)
    return O.fp8_e4m3_table()[codes].astype(F64) * s


_E2M1_CODE = {0.0: 0, 0.5: 1, 1.0: 2, 1.5: 3, 2.0: 4, 3.0: 5, 4.0: 6, 6.0: 7}


def encode_nvf4(w: np.ndarray):
    """[N, K] -> (codes uint8 [N, K/2], scale bytes uint8 [N, K/32]) in the engine's NK layout, written directly: per 32-column
    block a power-of-two scale byte (0x38 = 1.0 for a +-1 block) that puts the block's smallest non-zero entry at 1.0 - at 2.0,
    one exponent lower, on blocks with odd (row + block), so neighbours differ.  Exact or an error."""
    N, K = w.shape
    assert K % 32 == 0
    blocks = np.abs(w.astype(F64)).reshape(N, K // 32, 32)
    amax_all = float(np.abs(w).max()) or 1.0
    small = np.where(blocks > 0, blocks, np.inf).min(axis=2)
    small = np.where(np.isfinite(small), small, amax_all)
    odd = (np.arange(N)[:, None] + np.arange(K // 32)[None, :]) % 2
    e = np.log2(small) - odd
    assert np.array_equal(e, np.round(e)) and e.min() >= -7 and e.max() <= 8
    sbyte = ((e.astype(np.int64) + 7) << 3).astype(np.uint8)
    q = w.astype(F64).reshape(N, K // 32, 32) / (2.0 ** e)[:, :, None]
    mag = np.abs(q)
    assert np.isin(mag, list(_E2M1_CODE)).all(), "not exact in e2m1 under a power-of-two scale byte"
    codes = np.zeros(mag.shape, np.uint8)
    for val, c in _E2M1_CODE.items():
        codes[mag == val] = c
    codes = (codes | np.where(q < 0, 8, 0).astype(np.uint8)).reshape(N, K)
    data = (codes[:, 0::2] | (codes[:, 1::2] << 4)).astype(np.uint8)
    assert np.array_equal(NV.dequant_nk(data, sbyte).astype(F64), w.astype(F64))
    return data, sbyte


# ---- the probe ------------------------------------------------------------------------------------------------------------------

class Probe:
    """kind x shape x weight format (x vocabulary, x the H-wide slice of I a GU probe reads, x a leading pass-through layer)."""

    def __init__(self, kind: str, shape: str, fmt: str = "bf16", vocab: int = VOCAB, sl: int = 0, layers: int = 1, stair: bool = True):
        H, I, Hq, Hkv, D = SHAPES[shape]
        self.kind, self.shape, self.fmt, self.V, self.sl, self.L = kind, shape, fmt, vocab, sl, layers
        self.H, self.I, self.Hq, self.Hkv, self.D, self.G = H, I, Hq, Hkv, D, Hq // Hkv
        self.QD, self.NQ, self.NKV = Hq * D, Hq * D, Hkv * D
        self.NQKV = (Hq + 2 * Hkv) * D
        self.stair = stair and kind == "O" and fmt != "nvf4"
        self.cfg = dict(vocab_size=vocab, hidden_size=H, num_layers=layers, num_heads=Hq, num_kv_heads=Hkv, head_dim=D,
                        intermediate_size=I, rope_theta=THETA, norm_eps=EPS)
        seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(kind + shape))
        rng = np.random.default_rng(seed)
        erng = np.random.default_rng(H)                            # one embedding per width
        ids = np.arange(VOCAB)
        emb = erng.choice(np.array([-1.0, 1.0], F32), size=(VOCAB, H))
        emb[:, 0] = 1.0
        emb[:, 1:1 + NBITS] = np.where((ids[:, None] >> np.arange(NBITS)[None, :]) & 1, 1.0, -1.0)
        self.emb = emb[:vocab] if vocab <= VOCAB else None
        g_attn, g_mlp, g_fin = gammas(rng, H), gammas(rng, H), gammas(rng, H)
        g_attn[:1 + NBITS] = 1.0                                    # dimension 0 and the id bits reach Q / K unscaled
        g_mlp[0] = 1.0                                              # the gate's constant reads dimension 0
        wqkv, wo = np.zeros((self.NQKV, H), F32), np.zeros((H, self.QD), F32)
        wgu, wd = np.zeros((2 * I, H), F32), np.zeros((H, I), F32)
        lm = np.zeros((vocab, H), F32)
        lm[:H] = np.eye(H, dtype=F32)
        self.amplifier = 0.0
        if kind == "QL":
            wqkv = sparse_pm1(rng, self.NQKV, H, DENSITY["QL"])
            # every K and V row takes an ODD number of terms from the columns with |gamma| = 1 (the others are even): its sum is
            # odd, never zero.  A zero sum is the one integer whose fp32 evaluation on c32-scaled activations need not be exact
            # (the terms cancel to ~1e-6, and bf16 keeps that), so the cache stays comparable bit for bit on every path.
            odd_cols = np.flatnonzero(np.abs(g_attn) == 1.0)
            for r in range(self.NQ, self.NQKV):
                if np.count_nonzero(wqkv[r, odd_cols]) % 2 == 0:
                    c = odd_cols[np.flatnonzero(wqkv[r, odd_cols] == 0)[r % 7]]
                    wqkv[r, c] = 1.0 if r % 2 else -1.0
            lm = sparse_pm1(rng, vocab, H, DENSITY["LM"])
            # one exact duplicate of a token's winning row, 2048 rows away (a distant workgroup's range): the first token from
            # DUP_TOKEN on whose largest logit is a single integer
            m = (emb[:vocab] * g_fin) @ lm.T                        # float32: integer sums, exact
            top2 = np.partition(m, -2, axis=1)[:, -2:]
            self.dup_token = int(DUP_TOKEN + np.flatnonzero(top2[DUP_TOKEN:, 1] > top2[DUP_TOKEN:, 0])[0])
            win = int(np.argmax(m[self.dup_token]))
            other = win + DUP_SHIFT if win + DUP_SHIFT < vocab else win - DUP_SHIFT
            lm[other] = lm[win]
            self.dup = (min(win, other), max(win, other))
        elif kind == "O":
            wqkv[self.NQ + self.NKV:] = selection(self.NKV, H, 7, 29)
            wo = sparse_pm1(rng, H, self.QD, DENSITY["O"])
            if self.stair:
                s = 1.0
                while 2.0 * s * C64 * C64 / math.sqrt(D) * (1.0 - 2.0 ** -6) < MIN_STEP:
                    s *= 2.0
                self.amplifier = s
                cols = D // 2 - NBITS + np.arange(NBITS)           # the lowest RoPE frequencies
                for h in range(Hq):
                    wqkv[h * D + cols, 0] = s * 2.0 ** np.arange(NBITS)
                for h in range(Hkv):
                    wqkv[self.NQ + h * D + cols, 1 + np.arange(NBITS)] = 1.0
        elif kind in ("GUa", "GUb", "D"):
            n = np.arange(I)
            if kind == "GUa":
                gate = np.zeros((I, H), F32)
                for r in range(I):                                 # sparse +-1, clear of dimension 0's NVF4 scale block
                    c = rng.choice(np.arange(32, H), size=GATE_NNZ, replace=False)
                    gate[r, c] = rng.choice(np.array([-1.0, 1.0], F32), size=GATE_NNZ)
                gate[:, 0] = 64.0
                up = selection(I, H, 11, 3, mags=(1.0, 2.0, 1.0))
            elif kind == "GUb":
                gate = np.zeros((I, H), F32)
                gate[:, 0] = np.where((n * 7 + n // 3) % 3 == 0, 64.0, 32.0)
                up = sparse_pm1(rng, I, H, DENSITY["GUb"])
            else:
                gate = np.zeros((I, H), F32)
                gate[:, 0] = 32.0
                up = selection(I, H, 11, 3)
            wgu = np.concatenate([gate, up])
            if kind == "D":
                wd = sparse_pm1(rng, H, I, DENSITY["D"]) * F32(2.0 ** -5)
            else:
                lo = min(sl * H, I - H)                            # the last slice ends at I
                self.slice0 = lo
                j = np.arange(H)
                wd[j, lo + j] = np.where((j * 3 + j // 11) % 4 == 0, -1.0, 1.0) * 2.0 ** -5
        else:
            raise ValueError(kind)
        self.g_attn, self.g_mlp, self.g_fin = g_attn, g_mlp, g_fin
        self.w = {"w_qkv": wqkv, "w_o": wo, "w_gate_up": wgu, "w_down": wd}
        self.lm = lm
        # the leading pass-through layer of the two-layer variant: zero matrices, gammas of its own
        self.pass_gammas = (gammas(rng, H), gammas(rng, H)) if layers == 2 else None
        for a in (emb, lm, g_attn, g_mlp, g_fin, *self.w.values()):
            a.setflags(write=False)
        self.enc = None
        if fmt in ("fp8", "fp8a8"):
            self.enc = {k: encode_fp8(v) for k, v in self.w.items()}
        elif fmt == "nvf4":
            self.enc = {k: encode_nvf4(v) for k, v in self.w.items()}
        else:
            for v in self.w.values():
                assert np.array_equal(O.bf16_round(v), v)

    # ---- the float64 oracle on exactly the values the device holds ---------------------------------------------------------------
    def x(self, toks) -> np.ndarray:
        return self.emb[np.asarray(toks, np.int64)].astype(F64)

    def rope_tables(self, positions):
        """The engine's formula: fp32 frequency (a power of two at theta = 2**64), fp32 angle, double cos / sin, rounded to fp32."""
        i = np.arange(self.D // 2)
        freq = (2.0 ** (-64.0 * (2 * i) / self.D)).astype(F32)
        assert np.array_equal(freq.astype(F64), 2.0 ** (-64.0 * (2 * i) / self.D))
        ang = (np.asarray(positions, np.int64).astype(F32)[:, None] * freq[None, :]).astype(F32)
        return np.cos(ang.astype(F64)).astype(F32).astype(F64), np.sin(ang.astype(F64)).astype(F32).astype(F64)

    def forward(self, toks, positions, c_act: float = 1.0, hook=None, dtype=F64, reverse: bool = False, bf16_final: bool = False) -> dict:
        """Every readout of the live layer for `toks` at `positions`, row by row (own-row attention), in float64.
        c_act: the RMSNorm factor the projections' activations carry - 1.0 where they read bf16 rows, c where they read fp32
        rows.  The cache always holds the integers (bf16(c32 m) = m).  hook(name, W, X, Y) -> Y' mutates one projection's
        output (the sensitivity tests); hook(name + ".gamma", ...) the gamma in front of it.
        dtype = float32 (with `reverse`: every sum taken over K in the opposite order; bf16_final: the final normalised row
        rounded to bf16) turns the oracle into the emulation of a device path that tests/test_engine_linear_cpu.py holds
        against the bars."""
        hk = hook or (lambda name, W, X, Y: Y)
        H, D, half = self.H, self.D, self.D // 2
        T = dtype
        c_act = T(c_act)
        eps = T(EPS)

        def mm(X, Wm):
            return (X[:, ::-1] @ Wm[:, ::-1].T) if reverse else X @ Wm.T

        W = {k: v.astype(T) for k, v in self.w.items()}
        x = self.x(toks).astype(T)
        n = len(x)
        out = {}
        ga = hk("w_qkv.gamma", None, None, self.g_attn.astype(T))
        xa_i = x * ga                                                # integers +-1, +-2
        qkv_i = hk("w_qkv", W["w_qkv"], xa_i, mm(xa_i, W["w_qkv"]))
        k_i = qkv_i[:, self.NQ:self.NQ + self.NKV].reshape(n, self.Hkv, D)
        v_i = qkv_i[:, self.NQ + self.NKV:].reshape(n, self.Hkv, D)
        cos, sin = (t.astype(T) for t in self.rope_tables(positions))
        k1, k2 = k_i[..., :half], k_i[..., half:]
        out["k"] = c_act * np.concatenate([k1 * cos[:, None] - k2 * sin[:, None], k2 * cos[:, None] + k1 * sin[:, None]], -1)
        out["k_bar"] = c_act * 3 * U24 * np.concatenate([np.abs(k1 * cos[:, None]) + np.abs(k2 * sin[:, None])] * 2, -1) + BF16_U * np.abs(out["k"])
        out["k_int"], out["v"] = k_i, v_i
        attn = np.repeat(v_i, self.G, axis=1).reshape(n, self.QD)    # query head h reads kv head h // G; the cache holds integers
        o = hk("w_o", W["w_o"], attn, mm(attn, W["w_o"]))
        h1 = x + o
        out["o"] = o
        live_o = bool(self.w["w_o"].any())
        gm = hk("w_gate_up.gamma", None, None, self.g_mlp.astype(T))
        r1 = T(1.0) / np.sqrt((h1 * h1).mean(1, keepdims=True) + eps) if live_o else c_act
        xm = h1 * r1 * gm
        gu = hk("w_gate_up", W["w_gate_up"], xm, mm(xm, W["w_gate_up"]))
        g, u = gu[:, :self.I], gu[:, self.I:]
        act = hk("act", g, u, g / (T(1.0) + np.exp(-g)) * u)
        out["g"], out["u"], out["act"] = g, u, act
        d = hk("w_down", W["w_down"], act, mm(act, W["w_down"]))
        h2 = h1 + d
        out["d"], out["h2"] = d, h2
        out["rms"] = np.sqrt((h2 * h2).mean(1, keepdims=True) + eps)
        gf = hk("lm_head.gamma", None, None, self.g_fin.astype(T))
        passthrough = not (live_o or self.w["w_down"].any())
        xf = h2 * (c_act if passthrough else T(1.0) / out["rms"]) * gf
        if bf16_final:
            xf = O.bf16_round(xf.astype(F32)).astype(T)
        out["xf"] = xf
        lm = self.lm.astype(T)
        out["logits"] = hk("lm_head", lm, xf, mm(xf, lm))
        # accumulation terms sum_k |w_k x_k| of the projections that read fp32 activations
        out["abs_lm"] = np.abs(xf) @ np.abs(lm).T
        out["abs_o"] = np.abs(attn) @ np.abs(W["w_o"]).T
        out["abs_g"] = np.abs(xm) @ np.abs(W["w_gate_up"][:self.I]).T
        out["abs_u"] = np.abs(xm) @ np.abs(W["w_gate_up"][self.I:]).T
        out["abs_d"] = np.abs(act) @ np.abs(W["w_down"]).T
        return out

    # ---- bars ---------------------------------------------------------------------------------------------------------------------
    def norm_rel(self, n_bf16: int) -> float:
        """engine_stair_ref.logit_bar's relative part for this width."""
        return (1.0 + (self.H / 2 + 8) * U24) * (1.0 + BF16_U) ** n_bf16 - 1.0

    def ql_logit_bar(self, f: dict) -> np.ndarray:
        """fp32 logits of QL where lm_head reads fp32 activations: (K + 8) 2**-24 sum|w x| + (H/2 + 8) 2**-24 |ref|."""
        return (self.H + 8) * U24 * f["abs_lm"] + (self.H / 2 + 8) * U24 * np.abs(f["logits"])

    def readout_acc(self, f: dict, fp8_act: bool = False) -> np.ndarray:
        """|error| of h2 = x + ... [n, H] on a path whose projections read fp32 activations (GEMV chunks of 1 and 2
        sequences): (K + 8) 2**-24 sum|terms| per accumulation, carried through act = silu(g) u and the down projection.
        o_proj multiplies the cache's integers: exact in fp32 in any order, nothing is allowed - except on the fp8 x fp8 prefill
        (fp8_act), where every projection sums per-block integers times the product of two scales (the activations' row scale
        absmax / 448 is no power of two): at most three roundings per 128-column block, within the same (K + 8) 2**-24."""
        H, I = self.H, self.I
        e_g, e_u = (H + 8) * U24 * f["abs_g"], (H + 8) * U24 * f["abs_u"]
        e_act = e_g * np.abs(f["u"]) + e_u * np.abs(f["g"]) + 4 * U24 * np.abs(f["act"])
        e = e_act @ np.abs(self.w["w_down"].astype(F64)).T + (I + 8) * U24 * f["abs_d"]
        return e + (self.QD + 8) * U24 * f["abs_o"] if fp8_act else e

    def readout_bar(self, f: dict, n_bf16: int, fp32_act: bool, fp8_act: bool = False) -> np.ndarray:
        """Bound on |logits[:H] - want| of the O / GU / D readouts: the final norm and store (engine_stair_ref.logit_bar), one
        bf16 rounding where the lm_head reads bf16 rows, 2**-20 of the projection's own magnitude for a path that multiplies
        with c32 where the oracle has 1 or the reverse (the step's own V row may reach attention as fp32 c32 m or as the
        cache's m), and on fp32-activation paths the accumulation term.  Each error e of h2 moves its element by
        e |gamma| / rms and, through the row statistic, every element by at most |want| rms(e) / rms."""
        want = f["logits"][:, :self.H]
        e = 2.0 ** -20 * (np.abs(f["o"]) + np.abs(f["d"]))
        if fp32_act or fp8_act:
            e = e + self.readout_acc(f, fp8_act)
        return (self.norm_rel(n_bf16) * np.abs(want) + 1e-30 + e * np.abs(self.g_fin.astype(F64)) / f["rms"]
                + np.abs(want) * np.sqrt((e * e).mean(1, keepdims=True)) / f["rms"])

    # ---- preconditions of section 2 of the issue, asserted by the CPU test for every case the GPU test uses -------------------------
    def live_sums(self, f: dict) -> np.ndarray:
        if self.kind == "QL":
            return np.concatenate([f["k_int"].reshape(len(f["v"]), -1), f["v"].reshape(len(f["v"]), -1), f["logits"]], 1)
        return {"O": f["o"], "GUa": f["g"], "GUb": f["u"], "D": f["d"]}[self.kind]

    def check_conditions(self, toks, positions, rows=None, f=None, fc=None) -> dict:
        """The conditions of the module docstring for one case: the rows `rows` (default: all) of the forwards f (c_act = 1)
        and fc (c_act = c) of `toks` at `positions` (computed here when not given)."""
        f = f or self.forward(toks, positions, 1.0)
        fc = fc or self.forward(toks, positions, C64)
        rows = np.arange(len(f["v"])) if rows is None else np.asarray(rows)
        f, fc = ({k: v[rows] for k, v in d.items()} for d in (f, fc))
        s = self.live_sums(f)
        assert np.abs(s - np.round(s)).max() < 1e-9, "the live sums are not integers"     # float64 silu(32) = 32 (1 - 1.3e-14)
        s = np.round(s)
        assert np.abs(s).max() <= 256, (self.kind, self.shape, float(np.abs(s).max()))
        small_rows = (np.abs(s) < 128).reshape(len(s), -1).sum(1)          # per row, for the cases that are leading rows of this one
        frac = float(small_rows.sum() / s.size)
        assert frac >= 0.99, (self.kind, self.shape, frac)
        if self.kind == "GUa":
            assert s.min() >= 17, float(s.min())
        assert np.abs(f["v"]).max() <= 256 and np.abs(f["k_int"]).max() <= 256
        if self.kind in ("GUa", "GUb", "D"):
            # silu(g) = g in fp32 for every gate value, and act = g u is a small integer times a power of two: exact in bf16
            g32 = f["g"].astype(F32)
            assert np.array_equal(g32 / (F32(1.0) + np.exp(-g32)), g32) and np.array_equal(g32 * (F32(1.0) / (F32(1.0) + np.exp(-g32))), g32)
            a = f["g"] * f["u"]
            assert np.array_equal(O.bf16_round(a.astype(F32)).astype(F64), a), "act is not exact in bf16"
            assert (np.abs(f["act"] - a) <= U24 * np.abs(a)).all()        # (the float64 oracle keeps the true silu)
        # every element resolves an error of two units, and every accumulation bar is below half a unit term
        if self.kind == "QL":
            acc = float(self.ql_logit_bar(fc).max())
            assert acc < 0.5
        else:
            unit = {"O": 1.0, "GUa": 1.0 / 32, "GUb": 1.0, "D": 1.0}[self.kind]
            acc = float(self.readout_acc(fc).max())
            assert acc < 0.5 * unit, acc
            # two units of the live sum move an element of h2 by 2 unit x (the other factor >= 1): more than twice the widest bar,
            # wherever the element itself is below 128 (bf16 readout: 2**-8 relative)
            small = np.abs(f["h2"]) < 128
            bar = self.readout_bar(f, 1, False) * f["rms"] / np.abs(self.g_fin.astype(F64))       # in units of h2
            assert (bar[small] < 1.0).all(), float(bar[small].max())
        return {"max": float(np.abs(s).max()), "below128": frac, "acc": acc, "small_rows": small_rows, "per_row": s.size // len(s)}

    def check_rope(self, max_pos: int) -> None:
        """The staircase columns sit at frequencies 2**-(64 * 2 i / D), i >= D/2 - 12: cos rounds to 1.0f and sin stays below
        half an ulp of every other term at every position of the cache."""
        i = self.D // 2 - NBITS
        ang = (max_pos - 1) * 2.0 ** (-64.0 * 2 * i / self.D)
        assert F32(math.cos(ang)) == F32(1.0) and abs(math.sin(ang)) < 2.0 ** -25


@functools.lru_cache(maxsize=None)
def probe(kind: str, shape: str, fmt: str = "bf16", vocab: int = VOCAB, sl: int = 0, layers: int = 1, stair: bool = True) -> Probe:
    return Probe(kind, shape, fmt, vocab, sl, layers, stair)


def n_slices(shape: str) -> int:
    H, I = SHAPES[shape][:2]
    return -(-I // H)


@functools.lru_cache(maxsize=None)
def unique_top_tokens(kind: str, shape: str, vocab: int) -> tuple:
    """Token ids whose largest QL logit is a single integer (no tie), in ascending order."""
    p = probe("QL", shape, "bf16", vocab)
    m = (p.emb * p.g_fin) @ p.lm.T                                # float32: integer sums, exact
    top2 = np.partition(m, -2, axis=1)[:, -2:]
    return tuple(int(t) for t in np.flatnonzero(top2[:, 1] > top2[:, 0]) if t != p.dup_token)


def decode_tokens(kind: str, batch: int, shape: str = "W", vocab: int = VOCAB) -> list[int]:
    """Distinct tokens for the sequences of a step.  QL: tokens whose winning logit is unique (so the next token is decided by
    an integer margin on every path), except sequence 0, which takes the token with the planted duplicate row: there the two
    logits are bit-identical and the lower index must win."""
    if kind == "QL":
        pool = unique_top_tokens(kind, shape, vocab)
        return [probe("QL", shape, "bf16", vocab).dup_token] + [pool[(5 * s) % len(pool)] for s in range(1, batch)]
    return [(37 * s + 11) % vocab for s in range(batch)]


def decode_positions(kind: str, batch: int) -> list[int]:
    """O: position 0 for every sequence (one visible key).  Otherwise position s % 24: K rows meet real rotations, sequence 0 none."""
    return [0] * batch if kind == "O" else [s % 24 for s in range(batch)]


def prompt_tokens(n: int, start: int = 0, base: int = 1) -> list[int]:
    """Ascending ids (the O probe's staircase: row t returns its own V row), different in every row."""
    return [base + start + t for t in range(n)]


# ---- the cases of tests/test_engine_linear_gpu.py; tests/test_engine_linear_cpu.py asserts the conditions for every one of them -------
ALL = ("QL", "O", "GUa", "GUb", "D")
CACHE = 320
SWITCHES = ("PGK_FUSED_ATTN", "PGK_ATTN_MFMA", "PGK_MERGED_OPROJ", "PGK_BATCHED_MFMA", "PGK_BATCHED_MAX", "PGK_PACKED_PREFILL",
            "PGK_PACKED_DECODE", "PGK_FUSED_EPILOGUES", "PGK_GEMM256")


def _rig(shape, fmt="bf16", env=(), decode=(), replay=(), prefill=(), chunked=False, kinds=ALL, vocab=VOCAB, layers=1):
    return dict(shape=shape, fmt=fmt, env=tuple(env), decode=tuple(decode), replay=tuple(replay), prefill=tuple(prefill), chunked=chunked,
                kinds=tuple(kinds), vocab=vocab, layers=layers)


RIGS = {
    "W": _rig("W", decode=(1, 2, 3, 4, 5, 8, 16, 19, 33, 64), replay=(1, 4, 5, 33), prefill=(1, 17, 127, 128, 129, 257), chunked=True),
    "W-nofused": _rig("W", env=(("PGK_FUSED_ATTN", "0"),), decode=(1, 2, 33), replay=(2,)),
    "W-plain": _rig("W", env=(("PGK_FUSED_ATTN", "0"), ("PGK_MERGED_OPROJ", "0")), decode=(1, 2)),
    "W-ownoproj": _rig("W", env=(("PGK_MERGED_OPROJ", "0"),), decode=(2, 4)),
    "W-gemv": _rig("W", env=(("PGK_BATCHED_MFMA", "0"),), decode=(8, 3), replay=(8,)),
    "W-fp8-gemv": _rig("W", "fp8", env=(("PGK_BATCHED_MFMA", "0"),), decode=(8,)),
    "T-gemv": _rig("T", env=(("PGK_BATCHED_MFMA", "0"),), decode=(8,)),
    "W-mfma2": _rig("W", env=(("PGK_BATCHED_MFMA", "2"),), decode=(3, 4)),
    "W-nocopy": _rig("W", env=(("PGK_PACKED_PREFILL", "0"),), decode=(5, 16, 33), prefill=(1, 17, 127, 128)),
    "W-tiled": _rig("W", env=(("PGK_PACKED_DECODE", "0"),), decode=(19, 33, 64), replay=(33,)),
    "W-tiled-split": _rig("W", env=(("PGK_PACKED_DECODE", "0"), ("PGK_FUSED_ATTN", "0")), decode=(33,)),
    "W-max16": _rig("W", env=(("PGK_BATCHED_MAX", "16"),), decode=(19,)),
    "W-2layer": _rig("W", layers=2, decode=(1, 33), prefill=(17, 128)),
    "W-noepi": _rig("W", env=(("PGK_FUSED_EPILOGUES", "0"),), prefill=(129, 257)),
    "W-gemm256": _rig("W", env=(("PGK_GEMM256", "1"),), prefill=(257,)),
    "W-v4090": _rig("W", vocab=4090, kinds=("QL",), decode=(1, 2, 4, 5, 33), prefill=(17, 129)),
    "W-fp8": _rig("W", "fp8", decode=(1, 2, 4, 8, 6, 16, 19, 33), replay=(1, 6, 33), prefill=(17, 128, 129, 257)),
    "W-fp8-nofused": _rig("W", "fp8", env=(("PGK_FUSED_ATTN", "0"),), decode=(1, 2)),
    "W-fp8-nocopy": _rig("W", "fp8", env=(("PGK_PACKED_PREFILL", "0"),), decode=(19,), prefill=(17, 128, 129, 257)),
    # fp8 x fp8 prefill (prompts longer than 128): QL, O and D - their projection inputs are +-1, +-2 or +-32, +-64 per row, so
    # the row quantiser's e4m3 codes are exact; GU's integer act is not representable in e4m3
    "W-fp8a8": _rig("W", "fp8a8", kinds=("QL", "O", "D"), prefill=(129, 257)),
    "W-nvf4": _rig("W", "nvf4", decode=(1, 2, 4, 8, 5), replay=(1, 4), prefill=(17, 128, 129, 257)),
    "T": _rig("T", decode=(1, 2, 4, 8, 5, 12, 16), replay=(1, 5), prefill=(1, 17, 128, 129, 257)),
    "T-nocopy": _rig("T", env=(("PGK_PACKED_PREFILL", "0"),), decode=(5,), prefill=(17, 128)),
    "T-fp8": _rig("T", "fp8", decode=(1, 8, 5), prefill=(17, 129)),
    "T-nvf4": _rig("T", "nvf4", decode=(1, 4), prefill=(17,)),
    "X": _rig("X", decode=(1, 4, 5), prefill=(17,)),
    "W6": _rig("W6", decode=(1, 5), prefill=(17, 128)),
    "P": _rig("P", decode=(33,), replay=(33,), prefill=(17,)),
    "B4": _rig("B4", kinds=("GUa", "GUb", "D"), decode=(1, 4, 5)),
}
CHUNKED = (100, 50)            # one chunked prefill: 100 rows, then 50 at start_pos = 100


def rig_probes(rig: dict, kind: str) -> list:
    """The probes of one rig and kind: one per H-wide slice of I for the GU probes."""
    n = n_slices(rig["shape"]) if kind in ("GUa", "GUb") else 1
    return [probe(kind, rig["shape"], rig["fmt"], rig["vocab"], sl, rig["layers"]) for sl in range(n)]


def prefill_runs(rig: dict, kind: str, fmt: str) -> list:
    """(start, n) of every prefill call of a rig; the NVF4 O probe has no staircase and no prefill case."""
    if kind == "O" and fmt == "nvf4":
        return []
    runs = [[(0, n)] for n in rig["prefill"]]
    if rig["chunked"]:
        runs.append([(0, CHUNKED[0]), (CHUNKED[0], CHUNKED[1])])
    return runs


def argmax_lowest(logits: np.ndarray) -> np.ndarray:
    return np.argmax(logits, axis=-1)                               # NumPy returns the first maximum


# ---- planted errors (tests/test_engine_linear_cpu.py): hooks for Probe.forward ----------------------------------------------------
LIVE = {"QL": "w_qkv", "O": "w_o", "GUa": "w_gate_up", "GUb": "w_gate_up", "D": "w_down"}


def on(name, fn):
    """A hook that applies fn(W, X, Y) -> Y' to projection `name` only."""
    return lambda nm, W, X, Y: fn(W, X, Y.copy()) if nm == name else Y


def drop_columns(name, row: int, k0: int, width: int):
    """Row `row` loses its terms k0 .. k0 + width - 1: one term, or a 64-, 128- or 512-column k-chunk."""
    def fn(W, X, Y):
        Y[:, row] -= X[:, k0:k0 + width] @ W[row, k0:k0 + width]
        return Y
    return on(name, fn)


def tail_group(name, rows: int, stale: bool, n_end: int | None = None):
    """The last `rows` rows (ending at n_end, default N) left unwritten (zero) or all computed from the last row."""
    def fn(W, X, Y):
        e = Y.shape[1] if n_end is None else n_end
        Y[:, e - rows:e] = Y[:, e - 1:e] if stale else 0.0
        return Y
    return on(name, fn)


def neighbour_scale(name, fmt: str, row: int, kblock: int):
    """fp8: the 128 x 128 block at (row // 128, kblock) multiplied with the scale of block kblock + 1; NVF4: the 32-column block
    kblock of row `row` with the scale byte of block kblock + 1.  The encoders alternate the exponent, so the factor is 2 or 1/2."""
    def fn(W, X, Y):
        if fmt == "nvf4":
            factor = 2.0 if (row + kblock) % 2 == 0 else 0.5      # encode_nvf4: odd blocks carry the lower exponent
            k0, w, rows = kblock * 32, 32, slice(row, row + 1)
            factor = 1.0 / factor
        else:
            factor = 2.0 if (row // 128 + kblock) % 2 == 0 else 0.5   # encode_fp8: odd blocks carry the higher exponent
            k0, w, rows = kblock * 128, 128, slice(row // 128 * 128, row // 128 * 128 + 128)
        Y[:, rows] += (factor - 1.0) * (X[:, k0:k0 + w] @ W[rows, k0:k0 + w].T)
        return Y
    return on(name, fn)


def pair_shift():
    """Gate row n paired with up row n + 1."""
    return on("act", lambda g, u, act: g / (1.0 + np.exp(-g)) * np.roll(u, -1, axis=1))


def swap_rows(name, a: int, b: int):
    def fn(W, X, Y):
        Y[[a, b]] = Y[[b, a]]
        return Y
    return on(name, fn)


def slab(name, k0: int, k1: int, sign: float):
    """One split-K slab [k0, k1) dropped (sign -1) or added twice (+1)."""
    def fn(W, X, Y):
        return Y + sign * (X[:, k0:k1] @ W[:, k0:k1].T)
    return on(name, fn)


def gamma_shift(name):
    return on(name + ".gamma", lambda W, X, g: np.roll(g, 1))
