"""Exact per-element checks of the native engine's projections - w_qkv, w_o, w_gate_up, w_down, lm_head - on every linear path.

The probe models of tests/engine_linear_ref.py make ONE projection's every output readable through the unmodified engine
(prefill, set_state, decode_step, capture / replay, logits, all_logits, kv_cache, read_tokens; nothing is written behind its
back) while the other projections pass values through exactly.  Every readout is compared element by element with the float64
oracle on the values the device holds:

    KV cache      V rows on every path and K at position 0: bit for bit; K at later positions inside
                  3 * 2**-24 (|k1 cos| + |k2 sin|) + 2**-8 |ref| of the oracle's RoPE
    QL logits     all_logits (bf16) and every fp32 logit of a path that reads bf16 activations: the integer itself; fp32
                  activations (GEMV chunks of 1 and 2 sequences): (K + 8) 2**-24 sum|w x| + (H/2 + 8) 2**-24 |ref|
    QL next token the oracle's lowest-index argmax; sequence 0's winning lm_head row has an exact duplicate 2048 rows on
    O / GU / D    logits[:H] inside Probe.readout_bar (final norm + store, one bf16 rounding where the lm_head reads bf16
                  rows, the accumulation term on fp32-activation paths); logits[H:] exactly zero

The O probe decodes at position 0: one visible key, so whichever attention kernel the chunk takes - fused with o_proj, whole
context, split-KV with the merge kernel or the merged o_proj, GQA head chunks of 2 + 1 - must hand the step's own V row on
unchanged (probability exactly 1.0; the V row may reach it as fp32 c32 m or as the cache's m: 2**-20 of the projection's
magnitude is allowed for that, nothing else).  Every one of those kernels passes this element by element; none is exempt.

Which kernel ran is asserted through Engine.linear_plan / Engine.prefill_plan - the launchers' own decision functions - for
every branch named in EXPECT / PREFILL_EXPECT.  No whole-tensor norm ratio anywhere.  Out of reach: see engine_linear_ref."""

from __future__ import annotations

import contextlib
import os

import numpy as np
import pytest

from oracle import cpu_ref as O
from tests import engine_linear_ref as R

pytestmark = pytest.mark.gpu

pk = pytest.importorskip("pygpukit_amd")
from pygpukit_amd.core.dtypes import bfloat16  # noqa: E402
from pygpukit_amd.core.factory import from_numpy, zeros  # noqa: E402
from pygpukit_amd.llm import synthetic as S  # noqa: E402
from pygpukit_amd.llm.engine import Engine  # noqa: E402

F32, F64 = np.float32, np.float64
MAX_BATCH = 64


@contextlib.contextmanager
def switches(env):
    """The PGK_* switches of a rig, for the engine's construction and for every call (PGK_FUSED_EPILOGUES and PGK_GEMM256 are
    read per call); whatever the environment held is put back."""
    saved = {k: os.environ.pop(k, None) for k in R.SWITCHES}
    try:
        os.environ.update(dict(env))
        yield
    finally:
        for k in R.SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


_DEV: dict = {}
_RIGS: dict = {}


def device_weights(p):
    """The probe's arrays on the device, shared by every engine built on it."""
    key = (p.kind, p.shape, p.fmt, p.V, p.sl, p.L)
    if key not in _DEV:
        def mats(src, enc):
            out = {}
            for name, w in src.items():
                if enc is None:
                    out[name] = S._bf16(w)
                else:
                    out[name], out["s" + name[1:]] = from_numpy(enc[name][0]), from_numpy(enc[name][1])
            return out
        live = dict(attn_norm=S._bf16(p.g_attn), mlp_norm=S._bf16(p.g_mlp), q_norm=None, k_norm=None, **mats(p.w, p.enc))
        layers = [live]
        if p.L == 2:       # a leading layer of zero matrices with gammas of its own: the residual stream passes through
            zero = {k: np.zeros_like(v) for k, v in p.w.items()}
            enc = None if p.enc is None else {k: (R.encode_fp8 if p.fmt != "nvf4" else R.encode_nvf4)(v) for k, v in zero.items()}
            layers.insert(0, dict(attn_norm=S._bf16(p.pass_gammas[0]), mlp_norm=S._bf16(p.pass_gammas[1]), q_norm=None, k_norm=None, **mats(zero, enc)))
        _DEV[key] = (S._bf16(np.ascontiguousarray(p.emb)), layers, S._bf16(p.g_fin), S._bf16(p.lm))
    return _DEV[key]


class Rig:
    """One engine on one probe under one set of switches."""

    def __init__(self, rig_id: str, p):
        self.id, self.cfg, self.p = rig_id, R.RIGS[rig_id], p
        self.env = self.cfg["env"]
        emb, layers, fin, lm = device_weights(p)
        with switches(self.env):
            self.eng = Engine(p.cfg, emb, layers, fin, lm, max_seq_len=R.CACHE, max_batch=MAX_BATCH, weight_format=p.fmt, use_qk_norm=False)
        self.captured = 0

    # ---- cache rows of the live layer: (K words, V words) uint16 [Hkv, D] of row `pos` of slot s
    def cache_row(self, s: int, pos: int, n: int = 1):
        p = self.p
        out = []
        for c in self.eng.kv_cache(p.L - 1):
            out.append(np.stack([c._view(((s * p.Hkv + h) * R.CACHE + pos) * p.D, (n, p.D)).to_numpy() for h in range(p.Hkv)], axis=1))
        return out                                             # [n, Hkv, D] each

    def check_cache(self, kw, vw, f, rows, c_act, positions, what):
        """K / V words [n, Hkv, D] against rows `rows` of the oracle's forward f."""
        # values, not words: bf16 holds every integer up to 256 exactly, and a zero sum may carry either sign
        v = O.bf16_bits_to_f32(vw).astype(F64)
        bad = np.argwhere(v != f["v"][rows])
        assert not len(bad), (f"{what}: V differs from the integer at (row, kv head, element) {bad[:4].tolist()} of {len(bad)}: got "
                              f"{[v[tuple(b)] for b in bad[:4]]} want {[f['v'][rows][tuple(b)] for b in bad[:4]]}")
        k = O.bf16_bits_to_f32(kw).astype(F64)
        for i, r in enumerate(rows):
            if positions[r] == 0:
                bad = np.argwhere(k[i] != f["k_int"][r])
                assert not len(bad), (f"{what}: K at position 0 differs from the integer at (kv head, element) {bad[:4].tolist()} of {len(bad)}: got "
                                      f"{[k[i][tuple(b)] for b in bad[:4]]} want {[f['k_int'][r][tuple(b)] for b in bad[:4]]}")
            else:
                over = np.argwhere(np.abs(k[i] - f["k"][r]) > f["k_bar"][r])
                assert not len(over), f"{what}: row {r} position {positions[r]}: K outside its bar at (kv head, element) {over[:4].tolist()} of {len(over)}"

    def check_readout(self, got, f, rows, n_bf16, fp32_act, what):
        """fp32 logits got [n, V] of an O / GU / D probe against rows `rows` of f."""
        p = self.p
        want, bar = f["logits"][rows][:, :p.H], p.readout_bar(f, n_bf16, fp32_act, p.fmt == "fp8a8")[rows]
        assert np.isfinite(got).all(), f"{what}: non-finite logits"
        over = np.argwhere(np.abs(got[:, :p.H].astype(F64) - want) > bar)
        if len(over):
            r, c = over[0]
            raise AssertionError(f"{what}: {len(over)} elements outside the bar, first (row, element) ({r}, {c}): got {got[r, c]!r} want {want[r, c]!r} bar {bar[r, c]:.3g}")
        assert not got[:, p.H:].any(), f"{what}: logits beyond H are not zero at {np.argwhere(got[:, p.H:])[:4].tolist()}"

    # ---- one decode step of B sequences
    def step(self, B: int, replay: bool = False):
        p, eng = self.p, self.eng
        toks, pos = R.decode_tokens(p.kind, B, p.shape, p.V), R.decode_positions(p.kind, B)
        with switches(self.env):
            plan = eng.linear_plan(B, max(pos))
            eng.set_state(toks, pos)
            eng.reset_log()
            if replay:
                if self.captured != B:
                    eng.capture(B)
                    eng.set_state(toks, pos)
                    eng.reset_log()
                    self.captured = B
                eng.replay(1)
            else:
                eng.decode_step(B)
            eng.synchronize()
        logits = eng.logits(B).to_numpy().copy()
        nxt = eng.read_tokens(B, 1)[0].copy()
        rows = [self.cache_row(s, pos[s]) for s in range(B)]
        kw, vw = np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows])
        return plan, toks, pos, logits, nxt, kw, vw

    def check_step(self, B: int, replay: bool = False):
        p = self.p
        plan, toks, pos, logits, nxt, kw, vw = self.step(B, replay)
        what0 = (self.id, p.kind, p.fmt, "slice", p.sl, "batch", B, "replay" if replay else "eager")
        f_by = {}
        for ch in plan:
            fp32 = ch["act"] == "f32"
            c_act = R.C64 if fp32 else 1.0
            if c_act not in f_by:
                f_by[c_act] = p.forward(toks, pos, c_act)
            f = f_by[c_act]
            rows = np.arange(ch["b0"], ch["b0"] + ch["m"])
            what = what0 + ("chunk", ch["b0"], ch["form"], ch["m"])
            self.check_cache(kw[rows], vw[rows], f, rows, c_act, pos, what)
            if p.kind == "QL":
                got, want = logits[rows].astype(F64), f["logits"][rows]
                assert np.isfinite(got).all(), f"{what}: non-finite logits"
                bar = p.ql_logit_bar(f)[rows] if fp32 else np.zeros_like(want)
                over = np.argwhere(np.abs(got - want) > bar)
                assert not len(over), (f"{what}: {len(over)} logits outside the bar ({'fp32 accumulation' if fp32 else 'exact integers'}), first (row, index) "
                                       f"{over[0].tolist()}: got {got[tuple(over[0])]!r} want {want[tuple(over[0])]!r}")
                want_tok = R.argmax_lowest(f["logits"][rows])
                assert np.array_equal(nxt[rows], want_tok), f"{what}: next tokens {nxt[rows].tolist()} expected {want_tok.tolist()}"
                if ch["b0"] == 0:       # sequence 0: the planted duplicate - bit-identical logits, the lower index wins
                    lo, hi = p.dup
                    assert logits[0, lo] == logits[0, hi] and int(nxt[0]) == lo, f"{what}: duplicate rows {p.dup}: {logits[0, lo]!r} {logits[0, hi]!r} token {nxt[0]}"
            else:
                self.check_readout(logits[rows], f, rows, 0 if fp32 else 1, fp32, what)
        return plan, logits, nxt, kw, vw

    # ---- prefill calls [(start, n), ...] into slot `seq`
    def check_prefill(self, run, seq: int):
        p, eng = self.p, self.eng
        total = run[-1][0] + run[-1][1]
        toks, pos = R.prompt_tokens(total), list(range(total))
        f = p.forward(toks, pos, 1.0)
        plans = []
        for start, n in run:
            what = (self.id, p.kind, p.fmt, "slice", p.sl, "prefill", n, "at", start)
            buf = zeros((n, p.V), bfloat16)
            with switches(self.env):
                plans.append(eng.prefill_plan(n))
                last = eng.prefill(toks[start:start + n], seq=seq, start_pos=start, all_logits=buf)
                eng.synchronize()
            words = buf.to_numpy()
            rows = np.arange(start, start + n)
            kw, vw = self.cache_row(seq, start, n)
            self.check_cache(kw, vw, f, rows, 1.0, pos, what)
            if p.kind == "QL":
                bad = np.argwhere(O.bf16_bits_to_f32(words).astype(F64) != f["logits"][rows])
                assert not len(bad), f"{what}: all_logits differ from the integers at (row, index) {bad[:4].tolist()} of {len(bad)}"
                bad = np.argwhere(last.astype(F64) != f["logits"][rows[-1]])
                assert not len(bad), f"{what}: the last row's fp32 logits differ from the integers at {bad[:4].ravel().tolist()} of {len(bad)}"
            else:
                self.check_readout(O.bf16_bits_to_f32(words), f, rows, 1, False, what + ("all_logits",))
                self.check_readout(last[None, :], f, rows[-1:], 1, False, what + ("last row, fp32 GEMV lm_head",))
        return plans


def rigs_of(rig_id: str, kind: str) -> list:
    """Engines are built once per (rig, probe) per module."""
    out = []
    for p in R.rig_probes(R.RIGS[rig_id], kind):
        key = (rig_id, kind, p.sl)
        if key not in _RIGS:
            _RIGS[key] = Rig(rig_id, p)
        out.append(_RIGS[key])
    return out


@pytest.fixture(scope="module", autouse=True)
def _drop_engines():
    """The engines and weights go when the module is done, and the blocks they leave in the caching allocator go back to the
    driver: the fused matrices of the wide shape are 12 MiB, the very size class tests/test_stream.py takes for an unusual one
    that nobody else caches."""
    yield
    import gc

    from pygpukit_amd import _hip

    _RIGS.clear()
    _DEV.clear()
    gc.collect()
    _hip.call("pgk_stream_sync", None)
    _hip.call("pgk_pool_trim")


def look(plan, path: str):
    """plan entry by path: "<chunk>.<field>" or "<chunk>.proj.<name>.<field>"; a missing projection reads as None."""
    node = plan
    for part in path.split("."):
        if isinstance(node, list):
            node = node[int(part)]
        elif part not in node:
            return None
        else:
            node = node[part]
    return node


# ---- which branch every (rig, batch) must take, asserted through the plan -----------------------------------------------------
GEMV_W1 = {"0.form": "gemv", "0.m": 1, "0.act": "f32", "0.proj.qkv.kernel": "fused_gemv", "0.proj.qkv.r": 4, "0.proj.qkv.c": 2, "0.proj.gate_up.r": 6,
           "0.proj.gate_up.c": 2, "0.proj.gate_up.grid": 256, "0.proj.down.r": 1, "0.proj.down.c": 6, "0.proj.lm_head.r": 4, "0.proj.lm_head.grid": 1024}
BATCHED_W = {"0.form": "batched", "0.act": "bf16", "0.proj.qkv.kernel": "batched_reg", "0.proj.qkv.rows": 16, "0.proj.qkv.copy": 1, "0.proj.qkv.k": 1024,
             "0.proj.o.rows": 4, "0.proj.o.k": 2048, "0.proj.o.copy": 0, "0.proj.gate_up.rows": 16, "0.proj.gate_up.copy": 1, "0.proj.down.rows": 4,
             "0.proj.down.k": 3072, "0.proj.lm_head.kernel": "batched_reg", "0.proj.lm_head.rows": 16, "0.proj.lm_head.copy": 1}
PACKED_W = {"0.form": "packed", "0.carried": 1, "0.attn16": "direct", "0.proj.qkv.kernel": "pkgemm", "0.proj.o.kernel": "pkgemm_resid",
            "0.proj.down.kernel": "pkgemm_resid", "0.proj.lm_head.kernel": "batched_mt", "0.proj.lm_head.copy": 1}
EXPECT = {
    ("W", 1): {**GEMV_W1, "0.oproj": "fused", "0.proj.o": None, "0.proj.gate_up.pro": "norm_sum"},
    ("W", 2): {"0.form": "gemv", "0.m": 2, "0.act": "f32", "0.oproj": "own", "0.proj.o.r": 1, "0.proj.o.c": 4, "0.proj.gate_up.r": 2, "0.proj.gate_up.pro": "norm"},
    ("W", 3): {**BATCHED_W, "0.m": 3},
    ("W", 4): {"0.form": "gemv", "0.m": 4, "0.act": "bf16", "0.oproj": "own", "0.proj.qkv.r": 4, "0.proj.gate_up.r": 2},
    ("W", 5): {**BATCHED_W, "0.m": 5},
    ("W", 8): {**BATCHED_W, "0.m": 8},            # 5 sequences and more take the MFMA kernels: GEMV chunks of 8 need PGK_BATCHED_MFMA=0 (or NVF4)
    ("W-gemv", 8): {"0.form": "gemv", "0.m": 8, "0.act": "bf16", "0.oproj": "own", "0.proj.o.m": 8, "0.proj.o.act": "bf16", "0.proj.down.c": 6, "0.proj.qkv.r": 4},
    ("W-gemv", 3): {"0.form": "gemv", "0.m": 2, "1.form": "gemv", "1.m": 1, "1.b0": 2},
    ("W", 16): {**BATCHED_W, "0.m": 16},
    ("W", 19): {**PACKED_W, "0.m": 19, "0.proj.lm_head.tiles": 2},
    ("W", 33): {**PACKED_W, "0.m": 33, "0.proj.lm_head.tiles": 4},
    ("W", 64): {**PACKED_W, "0.m": 64, "0.proj.lm_head.tiles": 4},
    ("W-nofused", 1): {**GEMV_W1, "0.oproj": "merged", "0.proj.o": None, "0.proj.gate_up.pro": "norm_sum"},
    ("W-nofused", 2): {"0.form": "gemv", "0.m": 2, "0.oproj": "merged", "0.proj.o": None, "0.proj.gate_up.pro": "norm_sum"},
    ("W-nofused", 33): {"0.form": "packed", "0.attn16": "normrows"},
    ("W-plain", 1): {**GEMV_W1, "0.oproj": "own", "0.proj.o.r": 1, "0.proj.o.c": 4, "0.proj.o.m": 1, "0.proj.gate_up.pro": "norm"},
    ("W-plain", 2): {"0.form": "gemv", "0.m": 2, "0.oproj": "own", "0.proj.o.m": 2},
    ("W-ownoproj", 2): {"0.oproj": "own", "0.proj.o.m": 2, "0.proj.o.act": "f32"},
    ("W-ownoproj", 4): {"0.oproj": "own", "0.proj.o.m": 4, "0.proj.o.act": "bf16"},
    ("W-mfma2", 3): {"0.form": "batched", "0.m": 3},
    ("W-mfma2", 4): {"0.form": "batched", "0.m": 4, "0.proj.qkv.kernel": "batched_reg"},
    ("W-nocopy", 5): {"0.form": "batched", "0.proj.qkv.rows": 16, "0.proj.qkv.copy": 0, "0.proj.gate_up.copy": 0, "0.proj.lm_head.copy": 0},
    ("W-nocopy", 16): {"0.form": "batched", "0.m": 16, "0.proj.qkv.copy": 0},
    ("W-nocopy", 33): {"0.form": "tiled", "0.normrows": 1, "0.proj.qkv.kernel": "batched_mt", "0.proj.qkv.copy": 0, "0.proj.qkv.tiles": 4},
    ("W-tiled", 19): {"0.form": "tiled", "0.normrows": 1, "0.attn16": "direct", "0.proj.qkv.kernel": "batched_mt", "0.proj.qkv.rows": 16, "0.proj.qkv.copy": 1,
                      "0.proj.qkv.tiles": 2, "0.proj.o.rows": 4, "0.proj.down.rows": 4, "0.proj.gate_up.rows": 16},
    ("W-tiled", 33): {"0.form": "tiled", "0.proj.qkv.tiles": 4, "0.proj.lm_head.tiles": 4},
    ("W-tiled", 64): {"0.form": "tiled", "0.m": 64, "0.proj.down.tiles": 4},
    ("W-tiled-split", 33): {"0.form": "tiled", "0.attn16": "normrows", "0.normrows": 1},
    ("W-max16", 19): {"0.form": "batched", "0.m": 16, "1.form": "batched", "1.m": 3, "1.b0": 16},
    ("W-2layer", 1): {**GEMV_W1, "0.oproj": "fused"},
    ("W-2layer", 33): {**PACKED_W, "0.m": 33},
    ("W-v4090", 1): {"0.form": "gemv", "0.proj.lm_head.n": 4090, "0.proj.lm_head.grid": 1024},
    ("W-v4090", 2): {"0.form": "gemv", "0.m": 2},
    ("W-v4090", 4): {"0.form": "gemv", "0.act": "bf16"},
    ("W-v4090", 5): {"0.form": "batched", "0.proj.lm_head.copy": 0, "0.proj.lm_head.rows": 16, "0.proj.lm_head.grid": 256},
    ("W-v4090", 33): {"0.form": "packed", "0.proj.lm_head.kernel": "batched_mt", "0.proj.lm_head.copy": 0},
    ("W-fp8", 1): {"0.form": "gemv", "0.act": "f32", "0.oproj": "merged", "0.proj.qkv.w": "fp8", "0.proj.qkv.r": 4, "0.proj.qkv.c": 1, "0.proj.gate_up.r": 6,
                   "0.proj.gate_up.c": 1, "0.proj.down.c": 3, "0.proj.lm_head.w": "bf16", "0.proj.lm_head.c": 2},
    ("W-fp8", 2): {"0.form": "gemv", "0.oproj": "own", "0.proj.o.w": "fp8", "0.proj.o.c": 2, "0.proj.gate_up.r": 2},
    ("W-fp8", 4): {"0.form": "gemv", "0.act": "bf16", "0.proj.qkv.w": "fp8"},
    ("W-fp8", 8): {"0.form": "batched", "0.m": 8},
    ("W-fp8-gemv", 8): {"0.form": "gemv", "0.m": 8, "0.act": "bf16", "0.proj.qkv.w": "fp8", "0.proj.qkv.c": 1, "0.proj.down.c": 3},
    ("W-fp8", 6): {"0.form": "batched", "0.proj.qkv.kernel": "batched_reg", "0.proj.qkv.w": "fp8", "0.proj.qkv.copy": 0, "0.proj.lm_head.w": "bf16"},
    ("W-fp8", 16): {"0.form": "batched", "0.m": 16, "0.proj.down.w": "fp8"},
    ("W-fp8-nofused", 1): {"0.oproj": "merged", "0.proj.o": None},
    ("W-fp8-nofused", 2): {"0.oproj": "merged", "0.proj.o": None, "0.proj.gate_up.pro": "norm_sum"},
    ("W-fp8-nocopy", 19): {"0.form": "tiled", "0.proj.qkv.kernel": "batched_mt", "0.proj.qkv.w": "fp8", "0.proj.qkv.copy": 0},
    ("W-nvf4", 1): {"0.form": "gemv", "0.act": "f32", "0.oproj": "own", "0.proj.qkv.w": "nvf4", "0.proj.qkv.r": 4, "0.proj.qkv.c": 1, "0.proj.o.c": 2,
                    "0.proj.gate_up.r": 2, "0.proj.down.r": 1, "0.proj.down.c": 3, "0.proj.lm_head.w": "bf16"},
    ("W-nvf4", 2): {"0.form": "gemv", "0.m": 2, "0.act": "f32", "0.proj.qkv.r": 4},
    ("W-nvf4", 4): {"0.form": "gemv", "0.act": "bf16", "0.proj.qkv.r": 2, "0.proj.o.r": 2, "0.proj.gate_up.r": 2, "0.proj.down.r": 2, "0.proj.down.c": 3},
    ("W-nvf4", 8): {"0.form": "gemv", "0.m": 8, "0.proj.qkv.r": 2, "0.proj.qkv.c": 1},
    ("W-nvf4", 5): {"0.form": "gemv", "0.m": 4, "1.form": "gemv", "1.m": 1, "1.b0": 4, "1.act": "f32"},
    ("T", 1): {"0.form": "gemv", "0.oproj": "own", "0.proj.qkv.r": 1, "0.proj.qkv.c": 0, "0.proj.o.c": 0, "0.proj.gate_up.r": 2, "0.proj.gate_up.c": 0,
               "0.proj.down.c": 0, "0.proj.lm_head.c": 0, "0.proj.lm_head.r": 4},
    ("T", 2): {"0.form": "gemv", "0.m": 2, "0.proj.qkv.c": 0},
    ("T", 4): {"0.form": "gemv", "0.act": "bf16", "0.proj.qkv.c": 0},
    ("T", 8): {"0.form": "batched", "0.m": 8, "0.proj.qkv.mp": 8},
    ("T-gemv", 8): {"0.form": "gemv", "0.m": 8, "0.act": "bf16", "0.proj.down.c": 0, "0.proj.qkv.r": 1},
    ("T", 5): {"0.form": "batched", "0.proj.qkv.kernel": "batched_lds", "0.proj.qkv.mp": 8, "0.proj.o.kernel": "batched_lds", "0.proj.down.kernel": "batched_lds",
               "0.proj.lm_head.kernel": "batched_lds"},
    ("T", 12): {"0.form": "batched", "0.proj.qkv.kernel": "batched_lds", "0.proj.qkv.mp": 16},
    ("T", 16): {"0.form": "batched", "0.m": 16, "0.proj.gate_up.mp": 16},
    ("T-nocopy", 5): {"0.form": "batched", "0.proj.qkv.kernel": "batched_lds"},
    ("T-fp8", 1): {"0.form": "gemv", "0.proj.qkv.w": "fp8", "0.proj.qkv.c": 0, "0.proj.down.c": 0},
    ("T-fp8", 8): {"0.form": "batched", "0.proj.qkv.kernel": "batched_lds", "0.proj.qkv.w": "fp8", "0.proj.qkv.mp": 8},
    ("T-fp8", 5): {"0.form": "batched", "0.proj.qkv.kernel": "batched_lds", "0.proj.qkv.w": "fp8"},
    ("T-nvf4", 1): {"0.form": "gemv", "0.proj.qkv.w": "nvf4", "0.proj.qkv.c": 0, "0.proj.qkv.r": 1},
    ("T-nvf4", 4): {"0.form": "gemv", "0.proj.qkv.r": 2, "0.proj.qkv.c": 0},
    ("X", 1): {"0.form": "gemv", "0.oproj": "fused", "0.proj.qkv.r": 2, "0.proj.qkv.c": 1, "0.proj.gate_up.r": 2, "0.proj.gate_up.c": 1, "0.proj.down.c": 3},
    ("X", 4): {"0.form": "gemv", "0.act": "bf16", "0.proj.qkv.r": 2, "0.proj.o.c": 2, "0.proj.down.c": 3},
    ("X", 5): {"0.form": "batched", "0.proj.qkv.kernel": "batched_lds", "0.proj.o.kernel": "batched_reg", "0.proj.o.rows": 4, "0.proj.down.kernel": "batched_lds"},
    ("W6", 1): {"0.form": "gemv", "0.proj.gate_up.r": 6, "0.proj.gate_up.grid": 182, "0.proj.gate_up.n": 2176},
    ("W6", 5): {"0.form": "batched", "0.proj.gate_up.kernel": "batched_reg", "0.proj.gate_up.rows": 8, "0.proj.gate_up.copy": 0, "0.proj.down.kernel": "batched_lds"},
    ("P", 33): {"0.form": "packed", "0.carried": 0, "0.proj.o.kernel": "pkgemm", "0.proj.o.splits": 2, "0.proj.down.kernel": "pkgemm", "0.proj.down.splits": 8},
    ("B4", 1): {"0.form": "gemv", "0.proj.gate_up.r": 4, "0.proj.gate_up.c": 1, "0.proj.gate_up.n": 4096},
    ("B4", 4): {"0.form": "gemv", "0.act": "bf16", "0.proj.gate_up.r": 4},
    ("B4", 5): {"0.form": "batched", "0.proj.down.kernel": "batched_reg", "0.proj.down.rows": 4, "0.proj.down.k": 4096, "0.proj.gate_up.kernel": "batched_lds"},
}
# w8a16 engines hold the dequantised fragment-major copy, so their chunks of 17..64 sequences take the packed step as well
EXPECT[("W-fp8", 19)] = {"0.form": "packed", "0.m": 19}
EXPECT[("W-fp8", 33)] = {"0.form": "packed", "0.m": 33}

PREFILL_EXPECT = {
    ("W", 1): {"path": "pk", "pk_heads": 1, "carried": 1}, ("W", 17): {"path": "pk", "pk_heads": 1, "carried": 1}, ("W", 127): {"path": "pk"},
    ("W", 128): {"path": "pk", "carried": 1}, ("W", 129): {"path": "gemm", "fuse_heads": 1, "fuse_sw16": 1}, ("W", 257): {"path": "gemm", "fuse_heads": 1, "fuse_sw16": 1},
    ("W", 100): {"path": "pk"}, ("W", 50): {"path": "pk"},
    ("W-nocopy", 1): {"path": "ws", "pk": 0}, ("W-nocopy", 17): {"path": "ws"}, ("W-nocopy", 127): {"path": "ws"}, ("W-nocopy", 128): {"path": "ws"},
    ("W-2layer", 17): {"path": "pk", "carried": 1}, ("W-2layer", 128): {"path": "pk", "carried": 1},
    ("W-noepi", 129): {"path": "gemm", "fuse_heads": 0, "fuse_sw16": 0}, ("W-noepi", 257): {"path": "gemm", "fuse_heads": 0, "fuse_sw16": 0},
    ("W-gemm256", 257): {"path": "gemm", "fuse_heads": 0},
    ("W-v4090", 17): {"path": "pk"}, ("W-v4090", 129): {"path": "gemm"},
    ("W-fp8", 17): {"path": "pk"}, ("W-fp8", 128): {"path": "pk"}, ("W-fp8", 129): {"path": "gemm", "pkd": 1}, ("W-fp8", 257): {"path": "gemm", "pkd": 1},
    ("W-fp8-nocopy", 17): {"path": "ws", "pkd": 0}, ("W-fp8-nocopy", 128): {"path": "ws"}, ("W-fp8-nocopy", 129): {"path": "gemm", "pkd": 0},
    ("W-fp8-nocopy", 257): {"path": "gemm", "pkd": 0},
    ("W-fp8a8", 129): {"path": "fp8act", "fp8act": 1}, ("W-fp8a8", 257): {"path": "fp8act", "fp8act": 1},
    ("W-nvf4", 17): {"path": "ws", "nvf4": 1}, ("W-nvf4", 128): {"path": "ws", "nvf4": 1}, ("W-nvf4", 129): {"path": "gemm", "nvf4": 1},
    ("W-nvf4", 257): {"path": "gemm", "nvf4": 1},
    ("T", 1): {"path": "pk", "pk_heads": 0, "carried": 0}, ("T", 17): {"path": "pk", "pk_heads": 0, "carried": 0}, ("T", 128): {"path": "pk", "pk_heads": 0},
    ("T", 129): {"path": "gemm", "fuse_heads": 0}, ("T", 257): {"path": "gemm", "fuse_heads": 0},
    ("T-nocopy", 17): {"path": "ws"}, ("T-nocopy", 128): {"path": "ws"},
    ("T-fp8", 17): {"path": "pk"}, ("T-fp8", 129): {"path": "gemm"},
    ("T-nvf4", 17): {"path": "ws", "nvf4": 1},
    ("X", 17): {"path": "pk", "carried": 1},
    ("W6", 17): {"path": "ws", "pk": 0}, ("W6", 128): {"path": "ws", "pk": 0},      # K = 2176 has no split count the packed kernels take
    ("P", 17): {"path": "pk", "pk_heads": 1, "carried": 0},
}

# split-K slabs: the N = hidden projections of the 128-tile GEMMs (2 x 8 tiles: 4 slabs of K >= 512) and none on the 256-tile
# kernels; wsgemm_nt with slabs on every projection at the wide shape and WITHOUT a slab where K = 384 is one LDS tile;
# pkgemm_nt's slabs where no norm is carried; none on the in-staging-dequant fp8 GEMMs
for key, more in {("W", 129): {"s_o": 4, "s_d": 4, "s_qkv": 1}, ("W", 257): {"s_o": 4, "s_d": 4}, ("W-gemm256", 257): {"s_o": 1, "s_d": 1},
                  ("W-noepi", 257): {"s_o": 4, "s_d": 4}, ("W-nocopy", 17): {"s_qkv": 4, "s_o": 8, "s_gu": 2, "s_d": 12}, ("W-nocopy", 128): {"s_o": 8, "s_d": 12},
                  ("T", 17): {"s_o": 3, "s_d": 7}, ("T", 128): {"s_o": 3, "s_d": 7}, ("T-nocopy", 17): {"s_o": 1, "s_d": 2, "s_qkv": 2},
                  ("P", 17): {"s_o": 2, "s_d": 8}, ("W-fp8", 129): {"s_o": 4, "s_d": 4}, ("W-fp8-nocopy", 129): {"s_o": 1, "s_d": 1},
                  ("W-fp8-nocopy", 17): {"s_o": 8, "s_d": 12}, ("W-nvf4", 257): {"s_o": 4, "s_d": 4, "fuse_heads": 1, "fuse_sw16": 1}}.items():
    PREFILL_EXPECT[key].update(more)

DECODE_CASES = [(rid, kind) for rid, cfg in R.RIGS.items() if cfg["decode"] for kind in cfg["kinds"]]
PREFILL_CASES = [(rid, kind) for rid, cfg in R.RIGS.items() if cfg["prefill"] for kind in cfg["kinds"] if R.prefill_runs(cfg, kind, cfg["fmt"])]


def test_every_case_names_its_branch():
    for rid, cfg in R.RIGS.items():
        for B in cfg["decode"]:
            assert (rid, B) in EXPECT, (rid, B)
        for n in cfg["prefill"] + (R.CHUNKED if cfg["chunked"] else ()):
            assert (rid, n) in PREFILL_EXPECT, (rid, n)


@pytest.mark.parametrize("rig_id,kind", DECODE_CASES)
def test_decode_projection(rig_id, kind):
    """One eager step at every batch size of the rig, on every slice's engine: the plan names the branch, every element of the
    live projection is compared.  At the rig's replay sizes a captured, replayed step must give the eager step's bytes."""
    cfg = R.RIGS[rig_id]
    for r in rigs_of(rig_id, kind):
        for B in cfg["decode"]:
            plan, logits, nxt, kw, vw = r.check_step(B)
            for path, want in EXPECT[(rig_id, B)].items():
                assert look(plan, path) == want, (rig_id, B, path, want, look(plan, path), plan)
            if B in cfg["replay"]:
                _, logits2, nxt2, kw2, vw2 = r.check_step(B, replay=True)
                assert logits.tobytes() == logits2.tobytes() and np.array_equal(nxt, nxt2), (rig_id, kind, B, "a replayed step differs from the eager step")
                assert np.array_equal(kw, kw2) and np.array_equal(vw, vw2), (rig_id, kind, B, "a replayed step's cache rows differ from the eager step's")


@pytest.mark.parametrize("rig_id,kind", PREFILL_CASES)
def test_prefill_projection(rig_id, kind):
    """Every row of every prompt through all_logits and the cache, the last row also through the fp32 GEMV lm_head; one prompt
    in two chunks (start_pos > 0) where the rig asks for it."""
    cfg = R.RIGS[rig_id]
    for r in rigs_of(rig_id, kind):
        for i, run in enumerate(R.prefill_runs(cfg, kind, cfg["fmt"])):
            plans = r.check_prefill(run, seq=i % MAX_BATCH)
            for (start, n), plan in zip(run, plans):
                for k, want in PREFILL_EXPECT[(rig_id, n)].items():
                    assert plan[k] == want, (rig_id, n, k, want, plan)
