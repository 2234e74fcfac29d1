"""Per-element checks of the native engine's pointwise arithmetic - RMSNorm, QK-norm, RoPE, silu(g) u - on every path.

The probes of tests/engine_pointwise_ref.py (read its docstring for the bars, the rounding table and what is out of reach)
run through the unmodified engine - prefill, set_state, decode_step, capture / replay, logits, all_logits, kv_cache - one eager
step per case; at a rig's replay sizes a captured, replayed step must give the eager step's bytes.  Every element of every
readout is compared with the float64 oracle under the bar of the path the plan reports; which kernel ran is asserted through
linear_plan / prefill_plan (EXPECT, PREFILL_EXPECT).  No whole-tensor norm ratio anywhere.

Which case reaches which hand-written copy:
    RMSNorm   GEMV prologue PRO_NORM, register form            W 2, W-plain 1 (gate_up), every W gemv chunk's qkv / lm_head
              GEMV prologue PRO_NORM, LDS (generic-K) form     T 1, H5 1, 4, 19 (chunks of 8, 8, 2 and 1)
              GEMV prologue PRO_NORM_SUM                        W 1 (fused o_proj), W-nofused 2 (merged o_proj): NRo's o term
              batched_mfma_kernel / register-fragment kernel   T 5, T 8, X 5 / W 5, W-fp8 6
              M-tiled kernel's rows: norm_rows_bf16_kernel      W-tiled 19
              rmsnorm_f32_bf16_kernel<4>                        every prefill; its columns past 4096: H5 17, H5 129
              rmsnorm_f32_bf16_kernel<16>                       W-nocopy 17 and its single-token NRo prompt (8 and 12 slabs)
              carried statistics pkgemm_resid_nt -> pkgemm_nt   W 19, W 33 (decode), W 17 / 128 (prefill): the S probe's mlp_norm;
                                                                W-2layer 19 and 17: the second layer's attn_norm (K, V)
    QK-norm + RoPE + cache write
              new_token_finish                                  every decode chunk without the fused kernel (W 2 .. 33, T, X, P)
              the fused attention kernel's copy                 W 1, P 1 (oproj=fused)
              qknorm_rope_kvwrite_kernel<128>, <64>             W-noepi 129, W-gemm256 257, W-nocopy 17 (slabs) / T 17, T 129
              packed QKV epilogue                               W 17, W 128, chunked 100 + 50 (start_pos > 0), P 17
              qkv_head_finish                                   W 129 (bf16 128-tile), W-fp8 129 (dequantised copy)
    silu(g) u GEMV epilogue                                     W 1, 2, 4, W-gemv 8, T 1
              the three batched kernels                         W 5 (register), T 5 / 8 (LDS), W-tiled 19 (M-tiled)
              ops_pkgemm SwiGLU epilogue                        W 19, 33, W 17, 128
              swiglu_rows_kernel, with and without slabs        W-nocopy 17 (2 slabs), W-noepi 129
              fuse_sw16 GEMM epilogue                           W 129, W-fp8 129, T 129
              fuse_sw8 (with the e4m3 act)                      W-fp8a8-256 256
    The e4m3 outputs of rmsnorm_f32_bf16_kernel and swiglu_rows_kernel: W-fp8a8 129; the fp8 x fp8 GEMM's qkv_head_finish:
    W-fp8a8-256 256.
    Q (test_decode_q_through_scores) reaches the q side of new_token_finish and of the fused kernel's copy on every decode
    rig of the table; the prefill copies' q side is out of reach (engine_pointwise_ref).
    NRo's o term through split-K slabs: prompts of one token on T (3 slabs, <4>), P (2), W-nocopy and W-nvf4 (8, <16>); decode
    P 33 (2 slabs, the packed step's rmsnorm_slabs).  S's down term: W 129 (4 slabs), T 17 (7), W-nocopy 17 (12)."""

from __future__ import annotations

import numpy as np
import pytest

from oracle import cpu_ref as O
from tests import engine_pointwise_ref as R
from tests.test_engine_linear_gpu import look, switches

pytestmark = pytest.mark.gpu

pk = pytest.importorskip("pygpukit_amd")
from pygpukit_amd.core.dtypes import bfloat16  # noqa: E402
from pygpukit_amd.core.factory import from_numpy, zeros  # noqa: E402
from pygpukit_amd.llm import synthetic as S  # noqa: E402
from pygpukit_amd.llm.engine import Engine  # noqa: E402

F32, F64 = np.float32, np.float64
MAX_BATCH = 64
_RIGS: dict = {}


def outside(got, want, bar, what, names):
    """Assert |got - want| <= bar element by element; the message names the first offender and the worst ratio."""
    got = np.asarray(got, F64)
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    over = np.abs(got - want) / bar
    bad = np.argwhere(over > 1.0)
    if len(bad):
        i = tuple(bad[0])
        w = np.unravel_index(np.argmax(over), over.shape)
        raise AssertionError(f"{what}: {len(bad)} of {over.size} elements outside the bar; first at {names} {list(i)}: got {got[i]!r} want {want[i]!r} "
                             f"bar {bar[i]:.3g}; worst {over[w]:.3g} x the bar at {list(w)}: got {got[w]!r} want {want[w]!r}")


class Rig:
    """One engine on one probe under one set of switches."""

    def __init__(self, rig_id: str, p, max_seq: int = R.CACHE, max_batch: int = MAX_BATCH, env=None):
        self.id, self.p, self.max_seq = rig_id, p, max_seq
        self.env = R.RIGS[rig_id]["env"] if env is None else env

        def mats():
            out = {}
            for name, w in p.w.items():
                if p.enc is None:
                    out[name] = S._bf16(w)
                else:
                    out[name], out["s" + name[1:]] = from_numpy(p.enc[name][0]), from_numpy(p.enc[name][1])
            return out
        layers = [dict(attn_norm=S._bf16(p.g_attn), mlp_norm=S._bf16(p.g_mlp), q_norm=S._bf16(p.g_q), k_norm=S._bf16(p.g_k), **mats())]
        if p.L == 2:       # a leading layer of zero matrices with gammas of its own (bf16 rigs only): the stream passes through
            ga, gm, gq, gk = p.pass_gammas
            layers.insert(0, dict(attn_norm=S._bf16(ga), mlp_norm=S._bf16(gm), q_norm=S._bf16(gq), k_norm=S._bf16(gk),
                                  **{name: S._bf16(np.zeros_like(w)) for name, w in p.w.items()}))
        with switches(self.env):
            self.eng = Engine(p.cfg, S._bf16(np.ascontiguousarray(p.emb)), layers, S._bf16(p.g_fin), S._bf16(p.lm), max_seq_len=max_seq,
                              max_batch=max_batch, weight_format=p.fmt, use_qk_norm=p.qk_norm)
        self.captured = 0

    def cache_rows(self, s: int, pos: int, n: int = 1):
        p = self.p
        out = []
        for c in self.eng.kv_cache(p.L - 1):
            w = np.stack([c._view(((s * p.Hkv + h) * self.max_seq + pos) * p.D, (n, p.D)).to_numpy() for h in range(p.Hkv)], axis=1)
            out.append(O.bf16_bits_to_f32(w).astype(F64))
        return out                                              # K, V [n, Hkv, D]

    def check(self, f, rows, pos, path, k, v, logits, toks, what):
        p = self.p
        fr = {key: val[rows] if isinstance(val, np.ndarray) and val.shape[:1] == (len(pos),) and key != "freq" else val for key, val in f.items()}
        prow = [pos[r] for r in rows]
        outside(v, fr["v"], p.v_bar(fr, path), what + ("V cache",), "(row, kv head, element)")
        outside(k, fr["k"], p.k_bar(fr, path, prow), what + ("K cache",), "(row, kv head, element)")
        assert np.isfinite(logits).all(), f"{what}: non-finite logits"
        if p.kind == "S":
            outside(p.ratio(logits, [toks[r] for r in rows]), fr["h2"][:, p.half:], p.s_bar(fr, path), what + ("silu(g) u through the sentinel ratio",), "(row, column - H/2)")
        else:
            outside(logits[:, :p.H], fr["logits"], p.logit_bar(fr, path), what + ("logits",), "(row, index)")
        assert not logits[:, p.H:].any(), f"{what}: logits beyond H are not zero"

    def step(self, B: int, replay: bool = False, toks=None, pos=None):
        p, eng = self.p, self.eng
        toks = toks or R.decode_tokens(p.kind, B)
        pos = pos or R.decode_positions(p.kind, B)
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
        rows = [self.cache_rows(s, pos[s]) for s in range(B)]
        k, v = np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows])
        f = p.forward(toks, pos)
        for ch in plan:
            r = np.arange(ch["b0"], ch["b0"] + ch["m"])
            what = (self.id, p.kind, p.fmt, "slice", p.sl, "batch", B, "replay" if replay else "eager", "chunk", ch["b0"], ch["form"], ch["act"])
            self.check(f, r, pos, R.Path.decode(ch), k[r], v[r], logits[r], toks, what)
        return plan, logits, k, v

    def q_step(self, B: int, k: int):
        """Step k of the Q probe: fill every slot's cache through prefill, decode once, read the cache back for the oracle."""
        p, eng = self.p, self.eng
        toks, pos, prompts = R.q_case(p, B, k)
        with switches(self.env):
            for s, pr in enumerate(prompts):
                eng.prefill(pr, seq=s, want_last_logits=False)
            plan, aplan = eng.linear_plan(B, max(pos)), eng.attn_plan(B, max(pos))
            eng.set_state(toks, pos)
            eng.reset_log()
            eng.decode_step(B)
            eng.synchronize()
        logits = eng.logits(B).to_numpy().copy()
        rows = [self.cache_rows(s, 0, pos[s] + 1) for s in range(B)]
        for ch in plan:
            r = list(range(ch["b0"], ch["b0"] + ch["m"]))
            f = p.q_forward([toks[i] for i in r], [pos[i] for i in r], [rows[i][0] for i in r], [rows[i][1] for i in r], ch["act"] == "bf16", True,
                            R.Path.decode(ch).slabs)
            what = (self.id, "Q", p.fmt, "batch", B, "step", k, "chunk", ch["b0"], ch["form"], ch["act"], [a["attn"] for a in aplan])
            outside(logits[r][:, :p.H], f["logits"], f["bar"], what + ("logits through the softmax weights",), "(row, index)")
            assert not logits[r][:, p.H:].any(), f"{what}: logits beyond H are not zero"
        return plan

    def prefill(self, run, seq: int):
        p, eng = self.p, self.eng
        total = run[-1][0] + run[-1][1]
        toks, pos = R.prompt_tokens(total), list(range(total))
        f = p.forward(toks, pos)
        plans = []
        for start, n in run:
            what = (self.id, p.kind, p.fmt, "slice", p.sl, "prefill", n, "at", start)
            buf = zeros((n, p.V), bfloat16)
            with switches(self.env):
                plan = eng.prefill_plan(n)
                last = eng.prefill(toks[start:start + n], seq=seq, start_pos=start, all_logits=buf)
                eng.synchronize()
            plans.append(plan)
            rows = np.arange(start, start + n)
            k, v = self.cache_rows(seq, start, n)
            path = R.Path.prefill(plan)
            self.check(f, rows, pos, path, k, v, O.bf16_bits_to_f32(buf.to_numpy()), toks, what + ("all_logits",))
            self.check(f, rows[-1:], pos, path, k[-1:], v[-1:], last[None, :], toks, what + ("last row, fp32 GEMV lm_head",))
        return plans


def rigs_of(rig_id: str, kind: str) -> list:
    out = []
    for p in R.rig_probes(rig_id, kind):
        key = (rig_id, kind, p.sl)
        if key not in _RIGS:
            _RIGS[key] = Rig(rig_id, p)
        out.append(_RIGS[key])
    return out


@pytest.fixture(scope="module", autouse=True)
def _drop_engines():
    """The engines go when the module is done and their blocks go back to the driver (tests/test_engine_linear_gpu.py)."""
    yield
    import gc

    from pygpukit_amd import _hip

    _RIGS.clear()
    gc.collect()
    _hip.call("pgk_stream_sync", None)
    _hip.call("pgk_pool_trim")


DECODE_CASES = [(rid, kind) for rid, cfg in R.RIGS.items() if cfg["decode"] for kind in cfg["kinds"]]
PREFILL_CASES = [(rid, kind) for rid, cfg in R.RIGS.items() for kind in cfg["kinds"] if R.prefill_runs(rid, kind)]


@pytest.mark.parametrize("rig_id,kind", DECODE_CASES)
def test_decode_pointwise(rig_id, kind):
    cfg = R.RIGS[rig_id]
    for r in rigs_of(rig_id, kind):
        for B in cfg["decode"]:
            plan, logits, k, v = r.step(B)
            for path, want in R.EXPECT[(rig_id, B)].items():
                assert look(plan, path) == want, (rig_id, B, path, want, look(plan, path), plan)
            if B in cfg["replay"]:
                _, logits2, k2, v2 = r.step(B, replay=True)
                assert logits.tobytes() == logits2.tobytes(), (rig_id, kind, B, "a replayed step's logits differ from the eager step's")
                assert np.array_equal(k, k2) and np.array_equal(v, v2), (rig_id, kind, B, "a replayed step's cache rows differ from the eager step's")


@pytest.mark.parametrize("rig_id,kind", PREFILL_CASES)
def test_prefill_pointwise(rig_id, kind):
    for r in rigs_of(rig_id, kind):
        for i, run in enumerate(R.prefill_runs(rig_id, kind)):
            plans = r.prefill(run, seq=i % MAX_BATCH)
            for (start, n), plan in zip(run, plans):
                for key, want in R.PREFILL_EXPECT[(rig_id, n)].items():
                    assert plan[key] == want, (rig_id, n, key, want, plan)


@pytest.mark.parametrize("rig_id", list(R.Q_RIGS))
def test_decode_q_through_scores(rig_id):
    """Q's norm, RoPE, scale and head slots through the softmax weights of a decode step over 1 .. 5 cached keys."""
    (r,) = rigs_of(rig_id, "Q")
    for B in R.Q_RIGS[rig_id]:
        for k in range(R.q_steps(r.p, B)):
            plan = r.q_step(B, k)
            for path, want in R.EXPECT[(rig_id, B)].items():
                assert look(plan, path) == want, (rig_id, B, path, want, look(plan, path), plan)


def test_last_row_of_a_long_cache():
    """Position 4095 of a 4096-row cache on a max_batch-1 engine: the RoPE table's last row (a clamp one early reads row 4094),
    in one decode step and as the last row of a two-token prompt chunk at start_pos = 4094."""
    p = R.probe("NR", R.LONG["shape"], max_seq=R.LONG_CACHE)
    r = Rig("W", p, max_seq=R.LONG_CACHE, max_batch=1)
    r.step(1, toks=[20], pos=[R.LONG["pos"]])
    toks, pos = [21, 22], [R.LONG_CACHE - 2, R.LONG_CACHE - 1]
    f = p.forward(toks, pos)
    buf = zeros((2, p.V), bfloat16)
    with switches(r.env):
        plan = r.eng.prefill_plan(2)
        r.eng.prefill(toks, seq=0, start_pos=pos[0], all_logits=buf)
        r.eng.synchronize()
    k, v = r.cache_rows(0, pos[0], 2)
    r.check(f, np.arange(2), pos, R.Path.prefill(plan), k, v, O.bf16_bits_to_f32(buf.to_numpy()), toks, ("W", "NR", "prefill 2 at", pos[0]))
