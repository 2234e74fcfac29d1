"""Probe models that make the native engine's POINTWISE arithmetic - RMSNorm, per-head QK-norm, RoPE, silu(g) * u - readable
per element through the unmodified engine (NumPy only).

tests/engine_linear_ref.py and tests/engine_stair_ref.py reach exactness by switching this arithmetic off (+-1 embeddings,
rope_theta 2**64, no QK-norm, gates where silu(g) = g).  Here it is live and the projections are switched off instead: every
weight matrix is a SIGNED SELECTION - at most one non-zero per row, +-1 times a power of two, exact in bf16, in e4m3 under
power-of-two block scales and in NVF4 - so every readable number is a product chain through the live function, not a sum, and
its relative error is the sum of the relative roundings on its path.  The data are real-valued; the oracle (Probe.forward)
works in float64 on the values the device holds; every element of every readout is compared.

Probes (kind):
    "NR"   RMSNorm sites `attn_norm` and final norm, QK-norm and RoPE.  w_o = w_gate_up = w_down = 0, so the residual stream
           stays the embedding row x.  lm_head is a signed rotation of the first H rows: logits[j] = s_j xf[(j + H/2 + 1) % H],
           xf = final_norm(x) - the final norm itself, every column.  W_v is a signed selection: the V cache row holds
           attn_norm(x) at the columns (n mult + sl) % H, mult = H / (Hkv D) - one engine per slice `sl`, all H columns
           between them (H5: three of its 33 slices - every 33rd column from 0, 11 and 22 - and a fourth that reads the whole tail,
           columns 4096 .. 4223; the final-norm readout covers every column there).  W_k is a signed selection: the K cache row is
           rope(k_norm(selected attn_norm(x))), every kv head, every element, at the row's position.
    "NRo"  the same with a live o_proj: W_o is a signed selection that adds 2**e v[c] to every column of the stream, read
           through the final norm.  The step's own V row must reach o_proj unchanged, so the probe decodes at position 0 and
           prefills single-token prompts (one visible key, probability exactly 1.0).  The o_proj term arrives as split-K
           partials / slabs on the paths that have them: the PRO_NORM_SUM prologue and the slab-summing prefill norm must add
           every one of them (planted error "slab": one K range of o_proj dropped).
    "S"    silu(g) u and the `mlp_norm` site.  Embedding rows are non-zero in columns [0, H/2) only, column 0 (the sentinel)
           is exactly 1.0 (2**-10 on the rows t % 8 == 7, whose mean square is comparable to eps) and no projection writes it.  Gate row n reads the sentinel with weight GATE_W[n]: g = w xm[0]
           spans [-360, 45] over rows and tokens: 0, +-2**-6, either side of -88.7 (where fp32 exp(-g) overflows), beyond 17.
           Up row n is a signed selection of xm.  w_down writes 2**-3 act[lo + j] into stream column H/2 + j (one engine per
           H/2-wide slice of I).  The final norm's unknown factor cancels in logit ratios: with xf recovered from the
           logits, xf[c] / xf[0] * gf[0] / gf[c] = h2[c] / h2[0] = h2[c]  (4u allowed on the ratio).

    "Q"    q = rope(q_norm(selected attn_norm(x))) / sqrt(D), stored nowhere, read through the softmax weights of a decode
           step.  q and k dimension d read column 1 + d, v dimension d column 1 + D + d; token t's embedding is non-zero in the
           8 q / k columns of group t % (D / 8) only (4 rotate-half pairs) and in every v column, so one wrong q element is an
           eighth of a score; the group rotates over sequences and steps.  Sequence s decodes at position 1 .. 5 behind that
           many cached keys of its own group (prefilled through the engine), W_o and lm_head as in NRo: the logits are
           final_norm(x + W_o sum_j p_j v_j).  The oracle takes K and V rows FROM THE DEVICE'S CACHE (they are checked by NR);
           only q, the scores, the softmax and P V are its own.  q_norm is a quarter of the usual size: scores of order 1.

Embedding rows of NR / NRo (token t): standard normal times 2**(t % 13 - 6) (rms 2**-6 .. 2**6 across tokens), except
t % 16 == 3: one outlier 2**10 times the rest; 5: a constant row; 7: mean square comparable to norm_eps (eps placement
decides the result); 9: mean square far below eps.  Gammas are real-valued (uniform in +-[0.5, 2], bf16), unequal, both
signs, and different for attn_norm, mlp_norm, the final norm, q_norm and k_norm.

Notation: u = 2**-24, B = 2**-8 (one bf16 rounding, tests/base_ops_ref.py HALF_ULP), nr(n) = (n/2 + 8) u (rmsnorm bar of
tests/base_ops_ref.py).

ROUNDING TABLE (what `Path` carries; each line is a rounding point found in the code)
    xhat   bf16 x^ where the projections read bf16 activations: decode chunks with act=bf16 (store_x<bf16> in the GEMV
           prologue, the norm kernels of the batched / tiled / packed steps), every prefill (rmsnorm_f32_bf16_kernel)      1 B
           - act=f32 (GEMV chunks of 1 and 2 sequences): the prologue keeps fp32                                            0
    carried  packed path with carried norms (pkgemm_resid_nt leaves bf16(h gamma), pkgemm_nt multiplies its fp32
           accumulator by 1 / rms and rounds): every mlp_norm, and the attn_norm of every layer but the first (the
           W-2layer rig: a pass-through layer in front, K and V read from the second).  bf16(h gamma) replaces xhat's
           rounding, the product with inv adds one u                                                                   1 B + u
    proj   prefill and the packed decode step round qkv and gate / up rows to bf16 before the head finish / SwiGLU
           (qknorm_rope_kvwrite_kernel and swiglu_rows_kernel read bf16; the fused epilogues round their accumulators:
           ops_pkgemm.hip `to_f(from_f<bf16>(acc))`): a selection of a bf16 x^ is bf16 already, so this adds nothing
           unless the accumulator was scaled by inv (carried)                                                    0, carried 1 B
    act    act = silu(g) u stored bf16 wherever the down projection reads bf16 rows (everything but act=f32)              1 B
    final  the final norm's x^ (bf16 unless act=f32); the logits are x^ times +-1: fp32 store and bf16 all_logits exact    1 B
    cache  K and V rows are stored bf16.  V = bf16(+-2**e x^): nothing on top of a bf16 x^; one B on an fp32 x^            <= 1 B
    fp8a8  the fp8 x fp8 prefill quantises x^ and act to e4m3 per (row, 128 columns), scale = amax / 448: `e8`, half a spacing
           (2**-4 of a normal number, 2**-10 scale below 2**-6), carried as an ABSOLUTE error through the QK-norm and silu

BARS
    V cache      |v| (nr(H) + B) (+ B + u where the attn norm is carried: the W-2layer rig, whose live layer is the second)
    final norm   |xf| (nr(H) + final B)
    NRo logits   Probe.readout_bar of engine_linear_ref, restated: e = error of h1 = x + o (the V rows' relative error times
                 |o|, u |h1| for the add, u (|x| + |o|) per slab or partial added - the plan's count, Path.slabs), moved through the norm as e |g| / rms + |want| rms(e) / rms
    K cache      k = rope(kn), kn = k_norm(ks), ks = the selected attn_norm values with relative error r_in = nr(H) + xhat B
                 (+ 2 u for the selection's power of two and sign: exact, nothing).  Through the QK-norm a common bound r_in on
                 the elements' relative errors moves each normalised element by at most 2 r_in (once itself, once through the
                 rms): r = 2 r_in + nr(D); without QK-norm r = r_in.  RoPE: 3 u (|k1 cos| + |k2 sin|) (two products, one add),
                 r (|k1 cos| + |k2 sin|) for the inputs, (|k1| + |k2|) pos freq 2**-22 for one ulp of powf and one of the
                 angle's product (NumPy's power and glibc's may differ there), and B |ref| for the store.
    S ratio      want = 2**-3 silu(g) u.  d_in = nr(H) + xhat B (carried: + B + u) reaches g and u alike.  Relative error of
                 silu: kappa(g) d_in with kappa(g) = |1 + g (1 - sigma(g))|, the condition number of silu; of u: d_in; of the
                 exponential: LIB_RTOL |act| + LIB_ATOL |u| (tests/base_ops_ref.py); the division and product 3 u; the act
                 store B; the ratio 4 u and two final-norm roundings (numerator and sentinel) 2 final B; 2**-126 for a
                 flushed subnormal.

    Q readout    |dq| = K's chain without the cache store, times 1 / sqrt(D) (one more u), + B |q| (q is bf16 before the scores:
                 engine_attn.hip.h new_token_finish).  Score j: sum_d |dq_d| |k_jd| + (D + 8) u sum_d |q_d k_jd| (bf16 products are
                 exact in fp32); d = the largest over the keys.  Weight p_j: p_j (e^{2d} - 1) + p_j (2 LIB_RTOL + (L + 16) u) +
                 LIB_ATOL for the exponentials, the L-term sum, the division and a split-KV merge, + 2 B p_j for the bf16
                 probabilities (numerator and denominator) of the kernels that multiply P V on packed bf16 pairs or MFMA
                 (engine_attn.hip.h:629, attn_core.hip.h:224; allowed on every decode kernel: at most).  Output:
                 sum_j dp_j |v_jd| + (L + 8) u sum_j p_j |v_jd|, + B where the chunk's activations are bf16.  Then as NRo.
                 Planted at this readout (Q_MUTATIONS): q normed with k_norm's gamma, q heads written one slot on, the scale
                 dropped, upper half's sign, interleaved pairing, table row pos + 1, RoPE before the norm.  cos / sin exchanged,
                 the frequency index and the D/2 mean move a score by less than 4 bars at the low-frequency groups; they are
                 claimed at K's readout, whose code Q shares.

PLANTED ERRORS (MUTATIONS; tests/test_engine_pointwise_cpu.py asserts each leaves the bar by 4x on an element of every
readout that claims it): eps dropped; eps outside the square root; mean over H - 128 columns; sum over the first 4096 of 4224
columns; gamma index shifted; attn / mlp / final gammas exchanged; q and k gammas exchanged; QK-norm mean over D/2; norm applied
to V; RoPE before the norm; interleaved pairing; upper half's sign flipped; cos and sin exchanged; frequency index off by one;
table row pos + 1 and pos - 1; table row clamped one early; one o_proj slab dropped; gate and up exchanged; gate n with up
n + 1; sigmoid(g) u; gelu for silu.  "silu as g (1 - sigma(-g)) without the overflow guard" is INDISTINGUISHABLE and not
planted: in fp32 the cancellation in 1 - 1 / (1 + e^g) costs at most 2**-24 |g| absolutely (6e-7 at g = -10, where e^g < 2**-24
the result is 0 against a true |g e^g| < 1e-6) - inside LIB_ATOL |u| everywhere.

Out of reach / not built here:
    Q in prefill: the Q probe decodes; its prompts only fill the cache.  A prompt row's scores run on the flash-prefill kernels,
             whose online-softmax rescaling has no bar derived here, so the in-place q heads of qknorm_rope_kvwrite_kernel and
             the packed / GEMM head epilogues are read on K's side only.  Q without QK-norm is not run either (un-normed
             scores of this probe saturate the softmax).
    fp8a8    runs NR and S (W-fp8a8 129, W-fp8a8-256 256); half an e4m3 spacing hides "mean over H - 128 columns" and "gelu
             for silu" at its S readout - they are claimed on every other path.  No NRo case (its prompts are single tokens,
             below the path's 129).
    S runs on the shapes W and T only (bf16, fp8 and fp8a8 weights).  NRo's prompts are single tokens, so the o term meets the
    slab-summing prefill norm at n = 1 only; longer prompts meet it with S's down term.

Positions: decode sequence s sits at position s % 24 (NRo: 0); prompts run from 0, one of them in two chunks (100 rows, then
50 at start_pos = 100); one max_batch-1 engine with a 4096-row cache decodes and prefills at position 4095, the table's last
row (planted error "table row clamped one early").  rope_theta is 1e6, and 1e4 on W-theta1e4 and T-theta1e4 (one rig per
head_dim); W-noqk runs without QK-norm.
"""

from __future__ import annotations

import functools
import math

import numpy as np

from oracle import cpu_ref as O
from tests import base_ops_ref as BO
from tests import engine_linear_ref as L

F32, F64 = np.float32, np.float64
EPS = 1e-6
U = 2.0 ** -24
B16 = BO.HALF_ULP["bf16"]
LIB_RTOL, LIB_ATOL = BO.LIB_RTOL, BO.LIB_ATOL
SHAPES = {**L.SHAPES, "H5": (4224, 256, 2, 1, 128)}
CACHE = 320
LONG_CACHE = 4096
SWITCHES = L.SWITCHES
encode_fp8, encode_nvf4 = L.encode_fp8, L.encode_nvf4
# gate weights on the sentinel: powers of two (exact in every weight format, NVF4's one-entry blocks included) and zero
GATE_W = (0.0, 2.0 ** -6, -2.0 ** -6, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 4.0, -4.0, 8.0, -8.0, 16.0, -16.0, -32.0, -64.0, -128.0, 0.125, -0.125)
V_SLICES = {"H5": (0, 11, 22, -1)}          # -1: the last Hkv D columns (H5: 4096 .. 4223, the whole tail)


def bf16(x):
    return O.bf16_round(np.asarray(x, F32))


def nr(n: int) -> float:
    return (n / 2 + 8) * U


def sel_rows(n_rows: int, k: int, mult: int, off: int, mags=(1.0, 2.0, 0.5)):
    """(columns, signed power-of-two weights) of a selection: row n reads column (n mult + off) % k."""
    n = np.arange(n_rows)
    sign = np.where((n * 5 + n // 7) % 3 == 0, -1.0, 1.0)
    mag = np.asarray(mags, F64)[(n + n // 5) % len(mags)]
    return (n * mult + off) % k, sign * mag


def dense(cols, w, k: int) -> np.ndarray:
    m = np.zeros((len(cols), k), F32)
    m[np.arange(len(cols)), cols] = w
    return m


class Path:
    """The rounding points of one device path (the table in the module docstring)."""

    def __init__(self, xhat: int, carried: bool = False, act: int = 1, final: int = 1, a8: bool = False, slabs: int = 16):
        self.xhat, self.carried, self.act, self.final, self.a8, self.slabs = xhat, carried, act, final, a8, slabs

    @staticmethod
    def decode(chunk: dict) -> "Path":
        f32 = chunk["act"] == "f32"
        # additions that bring the o_proj term into the stream: the plan's split count where o_proj is a launch of its own; the
        # fused / merged o_proj leaves partials the plan does not count - at most 16, the engine's slab capacity
        o = chunk.get("proj", {}).get("o")
        slabs = int(o.get("splits", 1)) if o else 16
        return Path(0 if f32 else 1, bool(chunk.get("carried", 0)), 0 if f32 else 1, 0 if f32 else 1, slabs=slabs)

    @staticmethod
    def prefill(plan: dict) -> "Path":
        return Path(1, bool(plan.get("carried", 0)), 1, 1, bool(plan.get("fp8act", 0)), slabs=int(plan.get("s_o", 1)))


def e8(x: np.ndarray) -> np.ndarray:
    """|error| of the e4m3 activation quantiser on bf16 rows x [n, K] (per row and 128 columns: scale = amax / 448, code = RNE
    e4m3 of x / scale): half a spacing of e4m3 at x / scale - 2**-4 of a normal number's binade (3 mantissa bits), 2**-10 below
    2**-6 (subnormal spacing 2**-9) - times the scale, plus 4 u for the fp32 division and product.  Computed on the oracle's
    x; the device's bf16 x is within B of it: (1 + 2 B)."""
    n, K = x.shape
    b = np.abs(x).reshape(n, K // 128, 128)
    amax = b.max(axis=2, keepdims=True)
    return ((np.maximum(2.0 ** -4 * b, 2.0 ** -10 * amax / 448.0) + 4 * U * b) * (1 + 2 * B16)).reshape(n, K)


def dequant8(x: np.ndarray) -> np.ndarray:
    """oracle.cpu_ref.quantize_fp8_rows and back (the float32 restatement of the fp8 x fp8 prefill's activations)."""
    codes, scale = O.quantize_fp8_rows(np.asarray(x, F32))
    return (O.fp8_e4m3_table()[codes].astype(F64).reshape(x.shape[0], -1, 128) * scale.astype(F64)[:, :, None]).reshape(x.shape)


def silu64(g):
    with np.errstate(over="ignore"):
        return g / (1.0 + np.exp(-g))


SILU_MIN = -1.2784645427610738        # silu's only extremum: monotone on either side


class Probe:
    def __init__(self, kind: str, shape: str, fmt: str = "bf16", sl: int = 0, theta: float = 1e6, qk_norm: bool = True, max_seq: int = CACHE,
                 layers: int = 1):
        H, I, Hq, Hkv, D = SHAPES[shape]
        self.kind, self.shape, self.fmt, self.sl, self.theta, self.qk_norm, self.max_seq = kind, shape, fmt, sl, theta, qk_norm, max_seq
        self.L = layers
        self.H, self.I, self.Hq, self.Hkv, self.D, self.G = H, I, Hq, Hkv, D, Hq // Hkv
        self.QD, self.NKV = Hq * D, Hkv * D
        self.NQKV = (Hq + 2 * Hkv) * D
        self.V = max(4096, H)
        self.cfg = dict(vocab_size=self.V, hidden_size=H, num_layers=layers, num_heads=Hq, num_kv_heads=Hkv, head_dim=D, intermediate_size=I,
                        rope_theta=theta, norm_eps=EPS)
        rng = np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(shape)) + 977)

        def gamma(n):
            return bf16(rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n, p=[0.4, 0.6]))

        self.g_attn, self.g_mlp, self.g_fin, self.g_q, self.g_k = gamma(H), gamma(H), gamma(H), gamma(D), gamma(D)
        # the leading layer of the two-layer variant: zero matrices (the stream passes through), gammas of its own
        self.pass_gammas = (gamma(H), gamma(H), gamma(D), gamma(D)) if layers == 2 else None
        self.emb = self._embedding(kind == "S")
        self.half = H // 2
        # selections
        self.mult = max(1, H // self.NKV)
        self.vcol, self.vw = sel_rows(self.NKV, H, self.mult, sl)
        if sl < 0:
            self.vcol = H - self.NKV + np.arange(self.NKV)
        self.kcol, self.kw = sel_rows(self.NKV, H, 3 if H % 3 else 7, 5 + sl)
        self.qcol, self.qw = sel_rows(self.QD, H, 5 if H % 5 else 3, 2)
        if kind == "S":                                           # K, V, Q read the live lower half only
            self.vcol, self.kcol, self.qcol = self.vcol % self.half, self.kcol % self.half, self.qcol % self.half
        if kind == "Q":
            # q and k dimension d read column 1 + d (every head, its own signs and powers of two), v dimension d column 1 + D + d
            self.NG = D // 8                                      # groups of 8 dimensions: 4 rotate-half pairs
            self.qcol, self.kcol, self.vcol = (1 + np.arange(n_) % D + off for n_, off in ((self.QD, 0), (self.NKV, 0), (self.NKV, D)))
            self.g_q = bf16(self.g_q / 4)                         # scores of order 1: the softmax is not saturated
            self.emb = self._q_embedding()
        wqkv = np.concatenate([dense(self.qcol, self.qw, H), dense(self.kcol, self.kw, H), dense(self.vcol, self.vw, H)])
        wo, wgu, wd = np.zeros((H, self.QD), F32), np.zeros((2 * I, H), F32), np.zeros((H, I), F32)
        if kind in ("NRo", "Q"):
            self.ocol, self.ow = sel_rows(H, self.QD, 3 if self.QD % 3 else 5, 1, mags=(1.0, 0.5, 2.0, 0.25))
            wo = dense(self.ocol, self.ow, self.QD)
        if kind == "S":
            self.g_mlp = self.g_mlp.copy()
            self.g_mlp[0] = 1.0
            n = np.arange(I)
            self.gw = np.asarray(GATE_W, F64)[(n + n // len(GATE_W)) % len(GATE_W)]
            self.ucol, self.uw = sel_rows(I, self.half - 1, 7, 0)
            self.ucol = self.ucol + 1
            gate = np.zeros((I, H), F32)
            gate[:, 0] = self.gw
            wgu = np.concatenate([gate, dense(self.ucol, self.uw, H)])
            self.lo = min(sl * self.half, I - self.half)
            j = np.arange(self.half)
            self.dw = np.where((j * 3 + j // 11) % 4 == 0, -1.0, 1.0) * 2.0 ** -3
            wd[self.half + j, self.lo + j] = self.dw
        self.w = {"w_qkv": wqkv, "w_o": wo, "w_gate_up": wgu, "w_down": wd}
        j = np.arange(H)
        self.perm = (j + H // 2 + 1) % H
        self.lsign = np.where((j * 7 + j // 13) % 3 == 0, -1.0, 1.0)
        lm = np.zeros((self.V, H), F32)
        lm[j, self.perm] = self.lsign
        self.lm = lm
        self.enc = None
        if fmt in ("fp8", "fp8a8"):
            self.enc = {k: encode_fp8(v) for k, v in self.w.items()}
        elif fmt == "nvf4":
            self.enc = {k: encode_nvf4(v) for k, v in self.w.items()}
        for a in (self.emb, self.lm, self.g_attn, self.g_mlp, self.g_fin, self.g_q, self.g_k, *self.w.values()):
            a.setflags(write=False)

    def _embedding(self, sentinel: bool) -> np.ndarray:
        H, V = SHAPES[self.shape][0], self.V
        rng = np.random.default_rng(H * 7 + (1 if sentinel else 0))
        t = np.arange(V)
        e = rng.standard_normal((V, H))
        if sentinel:
            e *= np.asarray([0.5, 0.75, 1.0, 1.5, 2.0])[t % 5][:, None]
            e[:, H // 2:] = 0.0
            e[:, 0] = 1.0
            e[t % 8 == 7] *= 2.0 ** -10                           # sentinel 2**-10: mean square comparable to eps at the mlp_norm site
            return bf16(e)
        e *= (2.0 ** ((t % 13) - 6))[:, None]
        k = t % 16
        out = np.flatnonzero(k == 3)
        e[out] = rng.standard_normal((len(out), H)) * 2.0 ** -3
        e[out, (out * 7 + H - 64) % H] = 2.0 ** 7                  # (token 3: in the last 64 columns - past 4096 at H = 4224)
        const = np.flatnonzero(k == 5)
        e[const] = (0.75 * np.where(const // 16 % 2, -1.0, 1.0) * 2.0 ** (const // 32 % 3))[:, None]
        e[k == 7] = rng.standard_normal((int((k == 7).sum()), H)) * 1e-3
        e[k == 9] = rng.standard_normal((int((k == 9).sum()), H)) * 2.0 ** -20
        return bf16(e)

    def _q_embedding(self) -> np.ndarray:
        """Token t is non-zero in the 8 q / k columns of group t % NG (dimensions 4 g .. 4 g + 3 and their rotate-half partners)
        and in all D v columns: real values of order 1, different in every row."""
        H, D, V = self.H, self.D, self.V
        rng = np.random.default_rng(H * 11 + D)
        e = np.zeros((V, H))
        t = np.arange(V)
        g = t % self.NG
        for j in range(4):
            for off in (0, D // 2):
                e[t, 1 + 4 * g + j + off] = rng.uniform(0.5, 2.0, V) * rng.choice([-1.0, 1.0], V)
        e[:, 1 + D:1 + 2 * D] = rng.standard_normal((V, D))
        return bf16(e)

    def q_forward(self, toks, positions, K, V, act_bf16: bool, p_bf16: bool, slabs: int = 16, mut: str | None = None, emulate: bool = False) -> dict:
        """One decode step of the Q probe: sequence s sits at positions[s] and sees K[s], V[s] - the cache rows 0 .. positions[s]
        of its slot AS THE DEVICE HOLDS THEM (float64 [L, Hkv, D], its own row last) - so only q is the oracle's own:
        q = rope(q_norm(selected attn_norm(x))) / sqrt(D).  Returns the logits and their bar (see "Q readout" in the module
        docstring).  emulate: float32 with q, the probabilities and the attention output rounded to bf16."""
        T = F32 if emulate else F64
        n, D, half = len(toks), self.D, self.D // 2
        x = self.emb[np.asarray(toks, np.int64)].astype(T)
        xa = self._norm(x, self.g_attn, None, T, emulate)
        rope_mut = mut if mut in ("interleaved", "sign_flip", "cos_sin", "freq_off", "pos+1", "rope_first", "qk_half") else None
        cos, sin, freq = self.rope_tables(positions, rope_mut)
        qs = (xa[:, self.qcol] * self.qw.astype(T)).reshape(n, self.Hq, D)
        if mut == "head_slot":                                    # q head h written to slot h + 1
            qs = np.roll(qs, 1, axis=1)
        gq = None if not self.qk_norm else (self.g_k if mut == "qk_gamma" else self.g_q)
        q, qn = self._heads(qs, gq, cos, sin, rope_mut, T)
        scale = T(1.0) if mut == "no_scale" else T(1.0 / math.sqrt(D))
        q = q * scale
        if emulate:
            q = bf16(q).astype(T)
        # |error| of q: K's chain (k_bar) without the cache store, times the scale (one more u), then q's own bf16 rounding
        r_in = nr(self.H) + (B16 if act_bf16 else 0.0)
        r = 2 * r_in + nr(D) if self.qk_norm else r_in
        q1, q2 = np.abs(qn[..., :half]).astype(F64), np.abs(qn[..., half:]).astype(F64)
        c, sn = np.abs(cos)[:, None, :], np.abs(sin)[:, None, :]
        ang = (np.asarray(positions, F64)[:, None] * freq[None, :])[:, None, :] * 2.0 ** -22 * (q1 + q2)
        qb = ((r + 4 * U) * np.concatenate([q1 * c + q2 * sn, q2 * c + q1 * sn], -1) + np.concatenate([ang, ang], -1)) / math.sqrt(D) + B16 * np.abs(q.astype(F64))
        attn, e_attn = np.zeros((n, self.Hq, D), T), np.zeros((n, self.Hq, D))
        for s_ in range(n):
            L_ = len(K[s_])
            for h in range(self.Hq):
                Kh, Vh = K[s_][:, h // self.G, :].astype(T), V[s_][:, h // self.G, :].astype(T)
                sc = Kh @ q[s_, h]
                # scores: the products of two bf16 numbers are exact in fp32, their D-term sum is within (D + 8) u sum |q k|
                d = float((np.abs(Kh) @ qb[s_, h] + (D + 8) * U * (np.abs(Kh) @ np.abs(q[s_, h]))).max())
                w = np.exp(sc - sc.max())
                pr = w / w.sum()
                if emulate and p_bf16:
                    pr = bf16(w).astype(T) / bf16(w).astype(T).sum()
                # softmax: every score within d moves a weight by e^{2d} - 1 of itself; the exponential (LIB_RTOL, LIB_ATOL against a
                # denominator >= 1), the L-term sum and the division; bf16 probabilities (numerator and denominator) where used; a
                # split-KV merge rescales partials twice more (8 u)
                dp = pr.astype(F64) * (math.expm1(2 * d) + 2 * LIB_RTOL + (L_ + 16) * U + (2 * B16 if p_bf16 else 0.0)) + LIB_ATOL
                attn[s_, h] = pr @ Vh
                e_attn[s_, h] = dp @ np.abs(Vh).astype(F64) + (L_ + 8) * U * (pr.astype(F64) @ np.abs(Vh).astype(F64))
        if emulate and act_bf16:
            attn = bf16(attn).astype(T)
        a2 = attn.reshape(n, self.QD)
        o = a2[:, self.ocol] * self.ow.astype(T)
        e_o = (e_attn.reshape(n, self.QD)[:, self.ocol] + (B16 if act_bf16 else 0.0) * np.abs(a2[:, self.ocol]).astype(F64)) * np.abs(self.ow)
        h1 = x + o
        f = {"o": o.astype(F64), "h1": h1.astype(F64), "e_o": e_o, "q": q}
        f["rms"] = np.sqrt((f["h1"] ** 2).mean(1, keepdims=True) + EPS)
        f["xf"] = self._norm(h1, self.g_fin, None, T, emulate and act_bf16)
        f["logits"] = f["xf"][:, self.perm] * self.lsign.astype(T)
        if not emulate:
            f["bar"] = self.logit_bar(f, Path(1 if act_bf16 else 0, final=1 if act_bf16 else 0, slabs=slabs))
        return f

    # ---- the engine's RoPE table (engine.hip, pgk_engine_create): fp32 frequency, fp32 angle, double cos / sin rounded to fp32
    def rope_tables(self, positions, mut=None):
        i = np.arange(self.D // 2)
        expo = ((2 * i).astype(F32) / F32(self.D)).astype(F32)
        freq = (F32(1.0) / np.power(F32(self.theta), expo).astype(F32)).astype(F32)
        pos = np.asarray(positions, np.int64)
        if mut == "pos+1":
            pos = pos + 1
        elif mut == "pos-1":
            pos = np.maximum(pos - 1, 0)
        elif mut == "clamp_early":
            pos = np.minimum(pos, self.max_seq - 2)
        if mut == "freq_off":
            freq = np.roll(freq, -1)
        ang = (pos.astype(F32)[:, None] * freq[None, :]).astype(F32)
        cos, sin = np.cos(ang.astype(F64)).astype(F32).astype(F64), np.sin(ang.astype(F64)).astype(F32).astype(F64)
        return cos, sin, freq.astype(F64)

    def _norm(self, h, g, mut, T, rnd, carried=False):
        """x^ = h inv g.  rnd: round x^ to bf16.  carried: bf16(h g) first, then the product with inv (and, with rnd, the
        consumer's bf16 rounding)."""
        n = h.shape[1]
        eps = T(EPS)
        sq = h * h
        if mut == "mean_h128":
            ms = sq[:, :n - 128].sum(1, keepdims=True) / T(n - 128)
        elif mut == "sum_4096":
            ms = sq[:, :4096].sum(1, keepdims=True) / T(n)
        else:
            ms = sq.sum(1, keepdims=True) / T(n)
        if mut == "eps_dropped":
            inv = T(1.0) / np.sqrt(np.maximum(ms, T(1e-300) if T is F64 else T(1e-38)))
        elif mut == "eps_outside":
            inv = T(1.0) / (np.sqrt(ms) + eps)
        else:
            inv = T(1.0) / np.sqrt(ms + eps)
        g = g.astype(T)
        if mut == "gamma_shift":
            g = np.roll(g, 1)
        if carried:
            x = bf16(h * g).astype(T) * inv
        else:
            x = h * inv * g
        return bf16(x).astype(T) if rnd else x

    def _heads(self, x, gamma, cos, sin, mut, T):
        """[n, heads, D] -> (rope(norm(x)), the normalised k1, k2 halves)."""
        D, half = self.D, self.D // 2
        c, s = cos[:, None, :].astype(T), sin[:, None, :].astype(T)
        if mut == "cos_sin":
            c, s = s, c

        def norm(y):
            if gamma is None:
                return y
            ms = (y[..., :half] ** 2).mean(-1, keepdims=True) if mut == "qk_half" else (y * y).mean(-1, keepdims=True)
            return y * (T(1.0) / np.sqrt(ms + T(EPS))) * gamma.astype(T)

        def rope(y):
            if mut == "interleaved":
                y1, y2 = y[..., 0::2], y[..., 1::2]
                o = np.empty_like(y)
                o[..., 0::2], o[..., 1::2] = y1 * c - y2 * s, y2 * c + y1 * s
                return o
            y1, y2 = y[..., :half], y[..., half:]
            up = y2 * c - y1 * s if mut == "sign_flip" else y2 * c + y1 * s
            return np.concatenate([y1 * c - y2 * s, up], -1)

        kn = norm(x)
        out = norm(rope(x)) if mut == "rope_first" else rope(kn)
        return out, kn

    def forward(self, toks, positions, mut: str | None = None, T=F64, path: Path | None = None) -> dict:
        """Every readout for `toks` at `positions`, row by row (own-row attention), in dtype T.  path = None: the float64
        oracle, no roundings.  With T = float32 and a Path: the restatement with the roundings placed per the table."""
        p = path or Path(0, False, 0, 0)
        rnd = path is not None
        H, D, I = self.H, self.D, self.I
        n = len(toks)
        x = self.emb[np.asarray(toks, np.int64)].astype(T)
        ga, gm, gf = self.g_attn, self.g_mlp, self.g_fin
        if mut == "gamma_sites":
            ga, gm, gf = gm, gf, ga
        gq, gk = (self.g_q, self.g_k) if self.qk_norm else (None, None)
        if mut == "qk_gamma" and self.qk_norm:
            gq, gk = gk, gq
        out = {}
        ca = rnd and p.carried and self.L == 2                   # the live layer's attn_norm is carried from the layer before
        xa = self._norm(x, ga, mut, T, rnd and p.xhat and not ca, carried=ca)
        out["xa"] = xa
        if rnd and p.a8:
            xa = dequant8(xa).astype(T)
        cos, sin, freq = self.rope_tables(positions, mut)
        ks = (xa[:, self.kcol] * self.kw.astype(T)).reshape(n, self.Hkv, D)
        v = (xa[:, self.vcol] * self.vw.astype(T)).reshape(n, self.Hkv, D)
        if mut == "v_norm":
            v = v * (T(1.0) / np.sqrt((v * v).mean(-1, keepdims=True) + T(EPS))) * self.g_k.astype(T)
        if rnd and (p.a8 or ca):
            ks, v = bf16(ks).astype(T), bf16(v).astype(T)
        out["ks"] = ks
        k, kn = self._heads(ks, gk, cos, sin, mut, T)
        if rnd:
            k, v = bf16(k).astype(T), bf16(v).astype(T)
        out["k"], out["v"], out["kn"] = k, v, kn
        out["cos"], out["sin"], out["freq"] = cos, sin, freq
        h1 = x
        o = np.zeros_like(x)
        if self.kind == "NRo":
            attn = np.repeat(v, self.G, axis=1).reshape(n, self.QD)
            o = attn[:, self.ocol] * self.ow.astype(T)
            if mut == "slab":                                     # the K range [QD/4, QD/2) of o_proj dropped: one slab of 4, 8 or 12
                o = np.where((self.ocol >= self.QD // 4) & (self.ocol < self.QD // 2), T(0.0), o)
            h1 = x + o
        out["o"], out["h1"] = o, h1
        h2 = h1
        if self.kind == "S":
            xm = self._norm(h1, gm, mut, T, rnd and p.xhat and not p.carried, carried=rnd and p.carried)
            out["xm"] = xm
            if rnd and p.a8:
                xm = dequant8(xm).astype(T)
            g = xm[:, :1] * self.gw.astype(T)
            uu = xm[:, self.ucol] * self.uw.astype(T)
            if rnd and (p.carried or p.a8):
                g, uu = bf16(g).astype(T), bf16(uu).astype(T)
            if mut == "gate_up":
                g, uu = uu, g
            if mut == "pair_shift":
                uu = np.roll(uu, -1, axis=1)
            with np.errstate(over="ignore"):
                if mut == "sigmoid":
                    act = T(1.0) / (T(1.0) + np.exp(-g)) * uu
                elif mut == "gelu":
                    act = T(0.5) * g * (T(1.0) + np.tanh(T(BO.GELU_A) * (g + T(BO.GELU_B) * g * g * g))) * uu
                else:
                    act = g / (T(1.0) + np.exp(-g)) * uu
            if rnd and p.act:
                act = bf16(act).astype(T)
            if rnd and p.a8:
                act = dequant8(act).astype(T)
            out["g"], out["u"], out["act"] = g, uu, act
            d = np.zeros_like(x)
            d[:, self.half:] = act[:, self.lo:self.lo + self.half] * self.dw.astype(T)
            h2 = h1 + d
        out["h2"] = h2
        out["rms"] = np.sqrt((h2.astype(F64) ** 2).mean(1, keepdims=True) + EPS)
        xf = self._norm(h2, gf, mut, T, rnd and p.final)
        out["xf"] = xf
        out["logits"] = xf[:, self.perm] * self.lsign.astype(T)
        return out

    # ---- readouts and bars ----------------------------------------------------------------------------------------------------------
    def xf_from_logits(self, logits: np.ndarray) -> np.ndarray:
        xf = np.empty(logits[:, :self.H].shape, F64)
        xf[:, self.perm] = logits[:, :self.H].astype(F64) * self.lsign
        return xf

    def ratio(self, logits: np.ndarray, toks) -> np.ndarray:
        """S: h2[:, H/2:] recovered from the logits through the sentinel (h2[0] = the embedding's column 0, exactly)."""
        xf = self.xf_from_logits(logits)
        gf = self.g_fin.astype(F64)
        return xf[:, self.half:] / xf[:, :1] * gf[0] / gf[self.half:] * self.emb[np.asarray(toks, np.int64), :1].astype(F64)

    def attn_carried(self, p: Path) -> bool:
        return p.carried and self.L == 2

    def v_bar(self, f: dict, p: Path) -> np.ndarray:
        bar = np.abs(f["v"]) * (nr(self.H) + B16 + ((B16 + U) if self.attn_carried(p) else 0.0)) + 1e-38
        if p.a8:      # the quantised x^, the two scales' products (4 u) and the bf16 store of a value that is no longer bf16
            bar = bar + (np.abs(self.vw) * e8(f["xa"])[:, self.vcol]).reshape(bar.shape) + (B16 + 4 * U) * np.abs(f["v"])
        return bar

    def k_bar(self, f: dict, p: Path, positions) -> np.ndarray:
        half = self.D // 2
        r_in = nr(self.H) + p.xhat * B16 + ((B16 + U) if self.attn_carried(p) else 0.0)
        r = 2 * r_in + nr(self.D) if self.qk_norm else r_in
        k1, k2 = np.abs(f["kn"][..., :half]), np.abs(f["kn"][..., half:])
        c, s = np.abs(f["cos"])[:, None, :], np.abs(f["sin"])[:, None, :]
        lo, hi = k1 * c + k2 * s, k2 * c + k1 * s
        ang = (np.asarray(positions, F64)[:, None] * f["freq"][None, :])[:, None, :] * 2.0 ** -22 * (k1 + k2)
        bar = (r + 3 * U) * np.concatenate([lo, hi], -1) + np.concatenate([ang, ang], -1) + B16 * np.abs(f["k"]) + 1e-38
        if p.a8:
            # absolute errors e of the selected values (quantiser, scale products, bf16 qkv rounding) through the QK-norm:
            # d kn_i = g_i d ks_i / rms - kn_i d rms / rms with |d rms| <= rms(e), (1 + rms(e) / rms) for the second order
            e = (np.abs(self.kw) * e8(f["xa"])[:, self.kcol]).reshape(f["k"].shape) + (B16 + 4 * U) * np.abs(f["ks"])
            if self.qk_norm:
                rms = np.sqrt((f["ks"] ** 2).mean(-1, keepdims=True) + EPS)
                re = np.sqrt((e * e).mean(-1, keepdims=True)) / rms
                e = (e * np.abs(self.g_k.astype(F64)) / rms + np.abs(f["kn"]) * re) * (1 + re)
            e1, e2 = e[..., :half], e[..., half:]
            bar = bar + np.concatenate([e1 * c + e2 * s, e2 * c + e1 * s], -1)
        return bar

    def logit_bar(self, f: dict, p: Path) -> np.ndarray:
        """|logits[:H] - want|.  NR and S's sentinel-free columns: the final norm alone.  NRo: plus the error of h1 = x + o."""
        want = np.abs(f["logits"])
        bar = want * (nr(self.H) + p.final * B16) + 1e-38
        if self.kind in ("NRo", "Q"):
            e = f.get("e_o", np.abs(f["o"]) * (nr(self.H) + B16)) + U * np.abs(f["h1"]) + p.slabs * U * (np.abs(f["h1"] - f["o"]) + np.abs(f["o"]))
            g = np.abs(self.g_fin.astype(F64))
            em = e * g / f["rms"] + np.abs(f["xf"]) * np.sqrt((e * e).mean(1, keepdims=True)) / f["rms"]
            bar = bar + em[:, self.perm]
        return bar

    def s_bar(self, f: dict, p: Path) -> np.ndarray:
        sl = slice(self.lo, self.lo + self.half)
        g, uu, act = f["g"][:, sl], f["u"][:, sl], f["act"][:, sl]
        d_in = nr(self.H) + (p.xhat * B16 if not p.carried else 2 * B16 + U)
        with np.errstate(over="ignore"):
            kappa = np.abs(1.0 + g * (1.0 - 1.0 / (1.0 + np.exp(-g))))
        rel = kappa * d_in + d_in + LIB_RTOL + 3 * U + p.act * B16 + 4 * U + 2 * p.final * B16
        bar = 2.0 ** -3 * (rel * np.abs(act) + LIB_ATOL * np.abs(uu) * (1 + rel)) + 2.0 ** -126
        if p.a8:
            # x^ quantised: absolute errors eg, eu of gate and up (plus their bf16 rounding); silu over [g - eg, g + eg] moves by at
            # most its change at an end point or at its one extremum; act quantised again (e8 over the whole act row) and the
            # down projection's scale products (4 u)
            E = e8(f["xm"])
            eg = (np.abs(self.gw) * E[:, :1] + (B16 + 4 * U) * np.abs(f["g"]))
            eu = (np.abs(self.uw) * E[:, self.ucol] + (B16 + 4 * U) * np.abs(f["u"]))
            sg = silu64(f["g"])
            ds = np.maximum(np.abs(silu64(f["g"] + eg) - sg), np.abs(silu64(f["g"] - eg) - sg))
            ds = np.where(np.abs(f["g"] - SILU_MIN) < eg, np.maximum(ds, np.abs(silu64(SILU_MIN) - sg)), ds)
            ea = ds * (np.abs(f["u"]) + eu) + np.abs(sg) * eu
            ea = ea + e8(f["act"]) + e8(ea) + 4 * U * np.abs(f["act"])      # (the block's amax may itself be off by ea)
            bar = bar + 2.0 ** -3 * ea[:, sl]
        return bar


@functools.lru_cache(maxsize=None)
def probe(kind: str, shape: str, fmt: str = "bf16", sl: int = 0, theta: float = 1e6, qk_norm: bool = True, max_seq: int = CACHE,
          layers: int = 1) -> Probe:
    return Probe(kind, shape, fmt, sl, theta, qk_norm, max_seq, layers)


def slices(kind: str, shape: str) -> tuple:
    H, I, Hq, Hkv, D = SHAPES[shape]
    if kind == "Q":
        return (0,)
    if kind == "S":
        return tuple(range(-(-I // (H // 2))))
    return V_SLICES.get(shape, tuple(range(max(1, H // (Hkv * D)))))


SPECIAL = (7, 3, 5, 9)           # mean square ~ eps, outlier, constant, far below eps


def decode_tokens(kind: str, batch: int) -> list:
    """Sequences 0 .. 3 take the special rows (a batch of one decides eps placement), the rest distinct generic rows."""
    if kind == "S":
        return [7 if s == 0 else (37 * s + 11) % 4096 for s in range(batch)]
    return [SPECIAL[s] if s < 4 else (37 * s + 11) % 4096 for s in range(batch)]


def decode_positions(kind: str, batch: int) -> list:
    return [0] * batch if kind == "NRo" else [s % 24 for s in range(batch)]


def q_case(p: "Probe", batch: int, k: int = 0):
    """Step k of the Q probe at `batch` sequences: sequence s decodes a token of group (k batch + s) % NG at position
    1 + (s + k) % 5, behind that many cached keys of the same group (different rows): (tokens, positions, prompts)."""
    toks, pos, prompts = [], [], []
    for s in range(batch):
        g, L_ = (k * batch + s) % p.NG, 1 + (s + k) % 5
        toks.append(g + p.NG * (7 + s % 11))
        prompts.append([g + p.NG * (20 + 3 * s % 17 + i) for i in range(L_)])
        pos.append(L_)
    return toks, pos, prompts


def q_steps(p: "Probe", batch: int) -> int:
    """Steps until every group of 8 dimensions has been a query's (at most 4: a batch of one covers the first four groups and,
    through their rotate-half partners, 32 of the D dimensions)."""
    return min(4, -(-p.NG // batch))


def prompt_tokens(n: int, start: int = 0) -> list:
    return [1 + start + t for t in range(n)]


# ---- rigs: the switch sets of engine_linear_ref.RIGS, reduced to the cases of the issue's tables ---------------------------------------
def _rig(shape, base, decode=(), replay=(), prefill=(), chunked=False, kinds=("NR", "NRo", "S"), theta=1e6, qk_norm=True, env=(), layers=1):
    b = L.RIGS[base]
    return dict(shape=shape, fmt=b["fmt"], env=b["env"] + tuple(env), decode=tuple(decode), replay=tuple(replay), prefill=tuple(prefill), chunked=chunked,
                kinds=tuple(kinds), theta=theta, qk_norm=qk_norm, layers=layers)


RIGS = {
    "W": _rig("W", "W", decode=(1, 2, 4, 5, 19, 33), replay=(1, 4, 5, 33), prefill=(17, 128, 129), chunked=True),
    "W-theta1e4": _rig("W", "W", decode=(5,), prefill=(17,), kinds=("NR",), theta=1e4),
    "W-noqk": _rig("W", "W", decode=(1, 5, 33), prefill=(17, 129), kinds=("NR",), qk_norm=False),
    # a leading pass-through layer: the live layer's attn_norm arrives as carried statistics on the packed paths
    "W-2layer": _rig("W", "W", decode=(19,), prefill=(17,), kinds=("NR",), layers=2),
    "W-plain": _rig("W", "W-plain", decode=(1,)),
    "W-nofused": _rig("W", "W-nofused", decode=(2,), replay=(2,)),
    "W-tiled": _rig("W", "W-tiled", decode=(19,)),
    "W-gemv": _rig("W", "W-gemv", decode=(8,), replay=(8,)),
    "W-nocopy": _rig("W", "W-nocopy", prefill=(17,)),
    "W-noepi": _rig("W", "W-noepi", prefill=(129,)),
    "W-gemm256": _rig("W", "W-gemm256", prefill=(257,)),
    "T": _rig("T", "T", decode=(1, 5, 8), replay=(1, 5), prefill=(17, 129)),
    "T-theta1e4": _rig("T", "T", decode=(5,), prefill=(17,), kinds=("NR",), theta=1e4),
    "X": _rig("X", "X", decode=(5,), kinds=("NR", "NRo")),
    "P": _rig("P", "P", decode=(1, 33), replay=(33,), prefill=(17,), kinds=("NR", "NRo")),
    "W-fp8": _rig("W", "W-fp8", decode=(1, 6), replay=(1, 6), prefill=(129,)),
    "W-fp8a8": _rig("W", "W-fp8a8", prefill=(129,), kinds=("NR", "S")),
    # whole 256-row tiles on the 256-tile kernels: the fp8 x fp8 GEMMs' own head finish and SwiGLU + e4m3 epilogues
    "W-fp8a8-256": _rig("W", "W-fp8a8", prefill=(256,), kinds=("NR", "S"), env=(("PGK_GEMM256", "1"),)),
    "W-nvf4": _rig("W", "W-nvf4", decode=(1, 4), replay=(1, 4), prefill=(17,), kinds=("NR", "NRo")),
    "H5": _rig("H5", "W", decode=(1, 4, 19), prefill=(17, 129), kinds=("NR",)),
}
CHUNKED = L.CHUNKED
# the Q probe's decode cases (its prompts only fill the cache): rig -> batch sizes, the issue's decode table
Q_RIGS = {"W": (1, 2, 4, 5, 19, 33), "W-plain": (1,), "W-nofused": (2,), "W-tiled": (19,), "W-gemv": (8,), "T": (1, 5, 8), "X": (5,), "P": (1, 33),
          "W-fp8": (1, 6), "W-nvf4": (1, 4), "W-theta1e4": (5,)}
Q_MUTATIONS = ("qk_gamma", "head_slot", "no_scale", "sign_flip", "interleaved", "pos+1", "rope_first")
LONG = dict(shape="W", pos=LONG_CACHE - 1)      # the last row of a 4096-row cache on one max_batch-1 engine


def rig_probes(rig_id: str, kind: str) -> list:
    r = RIGS[rig_id]
    return [probe(kind, r["shape"], r["fmt"], sl, r["theta"], r["qk_norm"], layers=r["layers"]) for sl in slices(kind, r["shape"])]


def prefill_runs(rig_id: str, kind: str) -> list:
    """[(start, n), ...] per prefill call; NRo prefills single-token prompts only (its own V row must be the only key)."""
    r = RIGS[rig_id]
    if kind == "NRo":
        return [[(0, 1)]] if r["prefill"] else []
    runs = [[(0, n)] for n in r["prefill"]]
    if r["chunked"]:
        runs.append([(0, CHUNKED[0]), (CHUNKED[0], CHUNKED[1])])
    return runs


# ---- which branch every (rig, batch) / (rig, prompt length) takes: asserted through linear_plan / prefill_plan on the GPU -----------
GEMV1 = {"0.form": "gemv", "0.m": 1, "0.act": "f32"}
EXPECT = {
    ("W", 1): {**GEMV1, "0.oproj": "fused", "0.proj.gate_up.pro": "norm_sum"},
    ("W", 2): {"0.form": "gemv", "0.m": 2, "0.act": "f32", "0.oproj": "own", "0.proj.gate_up.pro": "norm"},
    ("W", 4): {"0.form": "gemv", "0.m": 4, "0.act": "bf16"},
    ("W", 5): {"0.form": "batched", "0.act": "bf16", "0.proj.qkv.kernel": "batched_reg"},
    ("W", 19): {"0.form": "packed", "0.carried": 1, "0.proj.qkv.kernel": "pkgemm", "0.proj.o.kernel": "pkgemm_resid"},
    ("W", 33): {"0.form": "packed", "0.carried": 1, "0.proj.lm_head.kernel": "batched_mt"},
    ("W-plain", 1): {**GEMV1, "0.oproj": "own", "0.proj.gate_up.pro": "norm"},
    ("W-nofused", 2): {"0.form": "gemv", "0.m": 2, "0.oproj": "merged", "0.proj.gate_up.pro": "norm_sum"},
    ("W-tiled", 19): {"0.form": "tiled", "0.normrows": 1, "0.proj.qkv.kernel": "batched_mt"},
    ("W-gemv", 8): {"0.form": "gemv", "0.m": 8, "0.act": "bf16"},
    ("T", 1): {"0.form": "gemv", "0.oproj": "own", "0.proj.qkv.c": 0},
    ("T", 5): {"0.form": "batched", "0.proj.qkv.kernel": "batched_lds"},
    ("T", 8): {"0.form": "batched", "0.m": 8},
    ("X", 5): {"0.form": "batched", "0.proj.qkv.kernel": "batched_lds", "0.proj.o.kernel": "batched_reg"},
    ("P", 1): {**GEMV1, "0.oproj": "fused", "0.proj.gate_up.pro": "norm_sum"},
    ("W-2layer", 19): {"0.form": "packed", "0.carried": 1, "0.proj.qkv.kernel": "pkgemm"},
    ("P", 33): {"0.form": "packed", "0.carried": 0, "0.proj.o.kernel": "pkgemm", "0.proj.o.splits": 2},
    ("W-fp8", 1): {"0.form": "gemv", "0.act": "f32", "0.oproj": "merged", "0.proj.qkv.w": "fp8"},
    ("W-fp8", 6): {"0.form": "batched", "0.proj.qkv.kernel": "batched_reg", "0.proj.qkv.w": "fp8"},
    ("W-nvf4", 1): {"0.form": "gemv", "0.act": "f32", "0.oproj": "own", "0.proj.qkv.w": "nvf4"},
    ("W-nvf4", 4): {"0.form": "gemv", "0.act": "bf16", "0.proj.qkv.r": 2},
}
# H5 (as the plan reports it: K = 4224 is outside the batched MFMA and packed kernels, so every chunk is a generic-K GEMV, at
# most 8 sequences each; its prompts take wsgemm_nt - QKV and gate / up in 9 slabs - and the 128-tile GEMMs with both epilogues)
EXPECT[("H5", 1)] = {**GEMV1, "0.oproj": "own", "0.proj.qkv.pro": "norm", "0.proj.qkv.c": 0, "0.proj.qkv.k": 4224, "0.proj.lm_head.c": 0}
EXPECT[("H5", 4)] = {"0.form": "gemv", "0.m": 4, "0.act": "bf16", "0.proj.qkv.c": 0}
EXPECT[("H5", 19)] = {"0.form": "gemv", "0.m": 8, "0.act": "bf16", "1.m": 8, "1.b0": 8, "2.m": 2, "2.act": "f32", "3.m": 1, "3.b0": 18}
for _rid in ("W-theta1e4", "W-noqk"):
    for _b in RIGS[_rid]["decode"]:
        EXPECT[(_rid, _b)] = EXPECT[("W", _b)]
EXPECT[("T-theta1e4", 5)] = EXPECT[("T", 5)]
PREFILL_EXPECT = {
    ("W", 1): {"path": "pk", "carried": 1}, ("W", 17): {"path": "pk", "pk_heads": 1, "carried": 1}, ("W", 128): {"path": "pk", "carried": 1},
    ("W", 129): {"path": "gemm", "fuse_heads": 1, "fuse_sw16": 1, "s_o": 4, "s_d": 4}, ("W", 100): {"path": "pk"}, ("W", 50): {"path": "pk"},
    ("W-nocopy", 1): {"path": "ws", "s_o": 8, "s_d": 12}, ("W-nocopy", 17): {"path": "ws", "s_qkv": 4, "s_o": 8, "s_gu": 2, "s_d": 12},
    ("W-noepi", 129): {"path": "gemm", "fuse_heads": 0, "fuse_sw16": 0}, ("W-noepi", 1): {"path": "pk"},
    ("W-gemm256", 257): {"path": "gemm", "fuse_heads": 0, "s_o": 1, "s_d": 1}, ("W-gemm256", 1): {"path": "pk"},
    ("W-2layer", 17): {"path": "pk", "pk_heads": 1, "carried": 1},
    ("T", 1): {"path": "pk", "pk_heads": 0, "carried": 0, "s_o": 3}, ("T", 17): {"path": "pk", "pk_heads": 0, "carried": 0, "s_o": 3, "s_d": 7},
    ("T", 129): {"path": "gemm", "fuse_heads": 0},
    ("P", 1): {"path": "pk", "carried": 0, "s_o": 2}, ("P", 17): {"path": "pk", "pk_heads": 1, "carried": 0, "s_o": 2, "s_d": 8},
    ("W-fp8", 1): {"path": "pk"}, ("W-fp8", 129): {"path": "gemm", "pkd": 1},
    ("W-fp8a8", 129): {"path": "fp8act", "fp8act": 1, "fuse_heads8": 0, "fuse_sw8": 0},
    ("W-fp8a8-256", 256): {"path": "fp8act", "fp8act": 1, "fuse_heads8": 1, "fuse_sw8": 1},
    ("W-nvf4", 1): {"path": "ws", "nvf4": 1, "s_o": 8}, ("W-nvf4", 17): {"path": "ws", "nvf4": 1},
}
PREFILL_EXPECT[("H5", 17)] = {"path": "ws", "pk": 0, "s_qkv": 9, "s_o": 1, "s_gu": 9, "s_d": 1}
PREFILL_EXPECT[("H5", 129)] = {"path": "gemm", "fuse_heads": 1, "fuse_sw16": 1, "s_o": 1, "s_d": 1}
for _rid in ("W-theta1e4", "W-noqk"):
    for _n in RIGS[_rid]["prefill"]:
        PREFILL_EXPECT[(_rid, _n)] = PREFILL_EXPECT[("W", _n)]
PREFILL_EXPECT[("T-theta1e4", 17)] = PREFILL_EXPECT[("T", 17)]

# ---- planted errors and the readouts that claim them ----------------------------------------------------------------------------------
NORM_MUTS = ("eps_dropped", "eps_outside", "mean_h128", "gamma_shift", "gamma_sites")
MUTATIONS = {
    "V": NORM_MUTS + ("v_norm",),
    "logits": NORM_MUTS,
    "K": ("qk_gamma", "qk_half", "rope_first", "interleaved", "sign_flip", "cos_sin", "freq_off", "pos+1", "pos-1"),
    "o": ("slab",),
    "S": NORM_MUTS + ("gate_up", "pair_shift", "sigmoid", "gelu"),
}
