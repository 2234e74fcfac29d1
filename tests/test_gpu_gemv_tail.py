"""The GEMV kernel's later trips and its lane-parallel tail, element by element (probes: tests/gemv_tail_ref.py).

No exact projection test ran a later trip of the GEMV lm_head before: every vocabulary fitted one pass of its 1024 x 16-row
grid, while the real model's 151 936 rows take nine or ten.  Here the QL probe of the benchmark's widths is decoded at
vocabularies of 1 - 2 and 2 - 3 trips per wave with a partial last row group, at decode batches 1, 2 and 4 (the M = 1, 2, 4
GEMV chunks) and on a w8a16 engine (its lm_head stays bf16; its layer GEMVs share the epilogue): every logit inside the
probe's derived bar (exact integers where the lm_head reads bf16 rows), K / V rows as in tests/test_engine_linear_gpu.py,
the next token the oracle's lowest-index argmax.  Four planted ties - duplicate rows in two lanes of one wave and trip, in
two waves of a workgroup, in two trips of one wave, in two workgroups - must each go to the lower row.  The epilogue's
partly filled last wave (gate/up at 3 pairs per wave, shape W6) and the residual epilogues are run at batches 1, 2 and 4."""

from __future__ import annotations

import numpy as np
import pytest

from tests import engine_linear_ref as R
from tests import gemv_tail_ref as T

pytestmark = pytest.mark.gpu

pk = pytest.importorskip("pygpukit_amd")
from pygpukit_amd.llm.engine import Engine  # noqa: E402
from tests import test_engine_linear_gpu as G  # noqa: E402

F64 = np.float64
MAX_BATCH = 4
_RIGS: dict = {}


class TailRig(G.Rig):
    """One engine on one TailProbe; the step takes its tokens from the caller."""

    def __init__(self, p):
        self.id, self.cfg, self.p, self.env = "tail", None, p, ()
        emb, layers, fin, lm = G.device_weights(p)
        with G.switches(self.env):
            self.eng = Engine(p.cfg, emb, layers, fin, lm, max_seq_len=R.CACHE, max_batch=MAX_BATCH, weight_format=p.fmt, use_qk_norm=False)
        self.captured = 0

    def run(self, toks, replay: bool = False):
        p, eng, B = self.p, self.eng, len(toks)
        pos = R.decode_positions("QL", B)
        plan = eng.linear_plan(B, max(pos))
        eng.set_state(toks, pos)
        eng.reset_log()
        if replay:
            eng.capture(B)
            eng.set_state(toks, pos)
            eng.reset_log()
            eng.replay(1)
        else:
            eng.decode_step(B)
        eng.synchronize()
        logits = eng.logits(B).to_numpy().copy()
        nxt = eng.read_tokens(B, 1)[0].copy()
        rows = [self.cache_row(s, pos[s]) for s in range(B)]
        kw, vw = np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows])
        assert len(plan) == 1 and plan[0]["form"] == "gemv" and plan[0]["m"] == B, plan
        lm = plan[0]["proj"]["lm_head"]
        assert lm["kernel"] == "fused_gemv" and lm["r"] == T.ROWS_PER_WAVE and lm["grid"] == T.GRID and lm["c"] > 0, lm
        fp32 = plan[0]["act"] == "f32"
        f = p.forward(toks, pos, R.C64 if fp32 else 1.0)
        what = (p.V, p.fmt, "batch", B, "replay" if replay else "eager")
        allrows = np.arange(B)
        self.check_cache(kw, vw, f, allrows, R.C64 if fp32 else 1.0, pos, what)
        got, want = logits.astype(F64), f["logits"]
        assert got.shape == want.shape and np.isfinite(got).all(), what
        bar = p.ql_logit_bar(f) if fp32 else np.zeros_like(want)
        err = np.abs(got - want)
        print(what, "max |logit error|", float(err.max()), "largest bar", float(bar.max()), "per trip:",
              [float(err[:, t * T.PASS:(t + 1) * T.PASS].max()) for t in range(-(-p.V // T.PASS))])
        over = np.argwhere(err > bar)
        assert not len(over), (f"{what}: {len(over)} logits outside the bar, first (row, index) {over[0].tolist()} (trip {over[0][1] // T.PASS}): "
                               f"got {got[tuple(over[0])]!r} want {want[tuple(over[0])]!r}")
        want_tok = R.argmax_lowest(f["logits"])
        assert np.array_equal(nxt, want_tok), f"{what}: next tokens {nxt.tolist()} expected {want_tok.tolist()}"
        return logits, nxt


def rig(vocab: int, fmt: str = "bf16") -> TailRig:
    if (vocab, fmt) not in _RIGS:
        _RIGS[(vocab, fmt)] = TailRig(T.tail_probe(vocab, fmt))
    return _RIGS[(vocab, fmt)]


@pytest.fixture(scope="module", autouse=True)
def _drop_engines():
    yield
    import gc

    from pygpukit_amd import _hip

    _RIGS.clear()
    G._RIGS.clear()
    G._DEV.clear()
    gc.collect()
    _hip.call("pgk_stream_sync", None)
    _hip.call("pgk_pool_trim")


@pytest.mark.parametrize("batch", [1, 2, 4])
@pytest.mark.parametrize("vocab", T.VOCABS)
def test_lm_head_later_trips(vocab, batch):
    """Every logit of every trip, the partial last row group included; a replayed step gives the eager step's bytes."""
    r = rig(vocab)
    toks = r.p.tokens(batch)
    logits, nxt = r.run(toks)
    logits2, nxt2 = r.run(toks, replay=True)
    assert logits.tobytes() == logits2.tobytes() and np.array_equal(nxt, nxt2)


@pytest.mark.parametrize("batch", [1, 4])
def test_lm_head_later_trips_w8a16(batch):
    """fp8 layer weights (their GEMVs end in the same epilogue), bf16 lm_head of two to three trips."""
    r = rig(T.V3, "fp8")
    r.run(r.p.tokens(batch))


@pytest.mark.parametrize("tie", list(T.TIES))
@pytest.mark.parametrize("vocab", T.VOCABS)
def test_argmax_tie_goes_to_the_lower_row(vocab, tie):
    """Duplicate rows at the maximal logit: bit-identical logits, the later copy never chosen - alone (batch 1) and as
    sequence 0 of a batch of 4."""
    r = rig(vocab)
    tok, lo, hi = r.p.ties[tie]
    for batch in (1, 4):
        logits, nxt = r.run(r.p.tokens(batch, first=tie))
        assert logits[0, lo] == logits[0, hi] == logits[0].max(), (tie, vocab, batch, logits[0, lo], logits[0, hi], logits[0].max())
        assert int(nxt[0]) == lo, (tie, vocab, batch, int(nxt[0]), lo, hi)


@pytest.mark.parametrize("kind", ["GUa", "GUb", "D", "O"])
def test_epilogue_lanes_at_the_edge(kind):
    """Shape W6: 2176 gate / up pairs at 3 pairs per wave (batch 1) leave the last live wave ONE output and the waves behind it
    none; batches 2 and 4 run the M = 2 and M = 4 epilogues (lanes m * OUT + r) on the same widths, and the D and O probes
    the residual epilogue.  Per element through the readouts of tests/test_engine_linear_gpu.py.  (Rows per wave of 1, 2 and
    4 divide every legal row count, so qkv, o_proj and down cannot have a partly filled last wave.)"""
    for r in G.rigs_of("W6", kind):
        for B in (1, 2, 4):
            plan, *_ = r.check_step(B)
            assert plan[0]["form"] == "gemv" and plan[0]["m"] == B, plan
    p = G.rigs_of("W6", kind)[0].p
    assert p.I % 3 == 1 and p.I % 12 != 0
