"""CPU side of the engine's exact projection checks (tests/engine_linear_ref.py; GPU side: tests/test_engine_linear_gpu.py).

1. Preconditions, for every (probe, shape, format, token set) the GPU test uses - they are conditions of the construction, not
   tolerances: the fp8 / NVF4 encodings reproduce the matrices exactly (asserted while the probe is built); every live sum is an
   integer within +-256 and at least 99 % of them are below 128; K and V sums of the QL probe are odd (never zero); gate values
   satisfy silu(g) = g in fp32 and act = g u is exact in bf16; every accumulation bar is below half a unit term and every
   readout element below 128 resolves one unit; the staircase of the O probe returns a prompt row's own V row with every other
   key at least 60 natural-log units below; the duplicate lm_head row ties exactly and no other token of a step has a tie.
2. The bars hold: a float32 emulation of every readout, in two summation orders, stays inside them.
3. Sensitivity: every planted error - one dropped term; a dropped 64-, 128-, 512-column k-chunk of one row; the last 4 / 16 / 64
   rows unwritten or computed from the last row; one fp8 scale block or NVF4 scale byte taken from its neighbour; gate row n
   paired with up row n + 1; two sequences' rows swapped; one split-K slab dropped or added twice; a gamma shifted by one
   column; the duplicate-row tie resolved to the higher index - falls outside the bars at the elements it touches.  The counts
   are printed (pytest -s)."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from oracle import cpu_ref as O
from tests import engine_linear_ref as R

F32, F64 = np.float32, np.float64
MAX_B = 64
MAX_PROMPT = max([n for cfg in R.RIGS.values() for n in cfg["prefill"]] + [sum(R.CHUNKED)])


def test_constants():
    R.check_constants()


# ---- 1. preconditions ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def forwards(kind: str, shape: str, vocab: int, sl: int, what: str, n: int):
    """(tokens, positions, forward with c_act = 1, forward with c_act = c) of the longest decode step / prompt: shorter ones are
    its leading rows (every row depends on its own token and position only)."""
    p = R.probe(kind, shape, "bf16", vocab, sl)
    if what == "decode":
        toks, pos = R.decode_tokens(kind, n, shape, vocab), R.decode_positions(kind, n)
    else:
        toks, pos = R.prompt_tokens(n), list(range(n))
    f = p.forward(toks, pos, 1.0)
    # the conditions that hold element by element are checked once, on the longest case; per case only the share below 128 remains
    cond = p.check_conditions(toks, pos, None, f, p.forward(toks, pos, R.C64))
    return toks, pos, f, cond


def share_below_128(cond: dict, n: int) -> float:
    return float(cond["small_rows"][:n].sum() / (n * cond["per_row"]))


def own_row_margin(p, toks) -> float:
    """The smallest lead, in natural-log units, of a prompt row's own key over every earlier key (float64 Q, K with RoPE)."""
    n = len(toks)
    xa = p.x(toks) * R.C64 * p.g_attn.astype(F64)
    qkv = xa @ p.w["w_qkv"].astype(F64).T
    cos, sin = p.rope_tables(range(n))
    half = p.D // 2

    def rope(t):
        t1, t2 = t[..., :half], t[..., half:]
        return np.concatenate([t1 * cos[:, None] - t2 * sin[:, None], t2 * cos[:, None] + t1 * sin[:, None]], -1)

    q = rope(qkv[:, :p.NQ].reshape(n, p.Hq, p.D))
    k = rope(qkv[:, p.NQ:p.NQ + p.NKV].reshape(n, p.Hkv, p.D))
    worst = np.inf
    for h in range(p.Hq):
        s = q[:, h] @ k[:, h // p.G].T / np.sqrt(p.D)
        lead = np.diag(s)[:, None] - s
        lead[np.triu_indices(n)] = np.inf                           # the row itself and the masked keys
        worst = min(worst, float(lead.min()))
    return worst


ALL_CASES = [(rid, kind) for rid, cfg in R.RIGS.items() for kind in cfg["kinds"]]


@pytest.mark.parametrize("rig_id,kind", ALL_CASES)
def test_preconditions(rig_id, kind):
    cfg = R.RIGS[rig_id]
    for pf in R.rig_probes(cfg, kind):                              # building it asserts the encoding of its format is exact
        p = R.probe(kind, cfg["shape"], "bf16", cfg["vocab"], pf.sl, 1, pf.stair)       # (the NVF4 O probe: the twin without a staircase)
        for name in p.w:
            assert np.array_equal(p.w[name], pf.w[name])            # one model in every format
        if cfg["decode"]:
            toks, pos, f, cond = forwards(kind, cfg["shape"], cfg["vocab"], pf.sl, "decode", MAX_B)        # (V and o do not depend on the staircase)
            assert len(set(toks)) == len(toks)
            for B in cfg["decode"]:
                assert share_below_128(cond, B) >= 0.99, (rig_id, kind, B)
                if kind == "QL":
                    lg = f["logits"][:B]
                    assert not (f["v"][:B] == 0).any() and not (f["k_int"][:B] == 0).any()
                    top = np.sort(lg, axis=1)
                    lo, hi = p.dup
                    assert lg[0, lo] == lg[0, hi] == top[0, -1] > top[0, -3] and int(np.argmax(lg[0])) == lo
                    assert (top[1:, -1] >= top[1:, -2] + 1).all()          # the other sequences: an integer margin
        runs = R.prefill_runs(cfg, kind, cfg["fmt"])
        if runs:
            toks, pos, f, cond = forwards(kind, cfg["shape"], cfg["vocab"], pf.sl, "prefill", MAX_PROMPT)
            for r in runs:
                assert share_below_128(cond, r[-1][0] + r[-1][1]) >= 0.99, (rig_id, kind, r)
            if kind == "O":
                assert pf.stair and p.stair
                p.check_rope(R.CACHE)
                assert own_row_margin(p, toks) >= R.MIN_STEP
        if kind == "O" and cfg["fmt"] == "nvf4":
            assert not pf.stair and not runs                        # out of reach: the staircase does not fit an NVF4 scale block


# ---- 2. and 3.: the readouts of one step, judged the way the GPU test judges them --------------------------------------------------

PATHS = {"bf16": (1.0, 1, False), "f32": (R.C64, 0, True)}        # c_act, bf16 roundings in front of the lm_head, fp32 accumulation


def outside(p, want: dict, got: dict, path: str, positions) -> dict:
    """Per readout, the mask of elements of `got` outside the bars around `want`."""
    c_act, n_bf16, fp32 = PATHS[path]
    at0 = (np.asarray(positions) == 0)[:, None, None]
    if p.kind == "QL":
        # the cache holds what a bf16 store leaves of c_act x the sum
        v = O.bf16_round((c_act * got["v"]).astype(F32)).astype(F64)
        k = O.bf16_round(got["k"].astype(F32)).astype(F64)
        return {"v": v != want["v"],
                "k": np.where(at0, k != want["k_int"], np.abs(k - want["k"]) > want["k_bar"]),
                "logits": np.abs(got["logits"] - want["logits"]) > (p.ql_logit_bar(want) if fp32 else 0.0)}
    bar = p.readout_bar(want, n_bf16, fp32)
    return {"logits": np.abs(got["logits"][:, :p.H] - want["logits"][:, :p.H]) > bar, "beyond": got["logits"][:, p.H:] != 0}


def touched(p, want: dict, got: dict) -> dict:
    """Per readout, the elements whose live-projection output the planted error changed."""
    if p.kind == "QL":
        return {"v": got["v"] != want["v"], "k": got["k_int"] != want["k_int"], "logits": got["logits"] != want["logits"]}
    if p.kind in ("O", "D"):
        key = "o" if p.kind == "O" else "d"
        return {"logits": np.abs(got[key] - want[key]) > 1e-9}
    a = np.abs(got["act"] - want["act"]) > 1e-9 * np.abs(want["act"]).max()
    return {"logits": a[:, p.slice0:p.slice0 + p.H]}


def step_of(kind, shape, sl=0, B=8):
    p = R.probe(kind, shape, "bf16", R.VOCAB, sl)
    toks, pos = R.decode_tokens(kind, B, shape), R.decode_positions(kind, B)
    return p, toks, pos


SENS_SHAPES = ("T", "W")
# Errors of one row must be caught at EVERY element they touch.  The others change many elements of a row at once, and with
# them the row's RMS, which the readout divides by: on a few elements the two changes cancel to within the bar (at most 4 % of
# the touched elements in any case here - a dropped slab of down_proj at K = 3072 on the fp32-activation path, whose
# accumulation bar is the widest), so they must be caught at 90 % of them.
WHOLE_ROW = ("one dropped term", "a dropped 64-column k-chunk", "a dropped 128-column k-chunk", "a dropped 512-column k-chunk",
             "one NVF4 scale byte from its neighbour")


@pytest.mark.parametrize("shape", SENS_SHAPES)
@pytest.mark.parametrize("kind", R.ALL)
def test_float32_emulation_stays_inside_the_bars(kind, shape):
    p, toks, pos = step_of(kind, shape, sl=R.n_slices(shape) - 1)
    for path, (c_act, n_bf16, fp32) in PATHS.items():
        want = p.forward(toks, pos, c_act)
        for reverse in (False, True):
            got = p.forward(toks, pos, R.C32 if fp32 else 1.0, dtype=F32, reverse=reverse, bf16_final=(n_bf16 == 1 and kind != "QL"))
            got = {k: np.asarray(v, F64) for k, v in got.items()}
            over = outside(p, want, got, path, pos)
            assert not any(m.any() for m in over.values()), (kind, shape, path, reverse, {k: int(m.sum()) for k, m in over.items()})


def planted(p, toks, pos):
    """(name, hook) of every planted error that applies to this probe's live projection."""
    live = R.LIVE[p.kind]
    N, K = p.w[live].shape
    half_of = {"GUa": 0, "GUb": p.I}.get(p.kind, 0)                 # the live half of w_gate_up starts here
    n_end = {"GUa": p.I, "GUb": 2 * p.I}.get(p.kind, N)              # ... and ends here
    if p.kind in ("GUa", "GUb"):
        row = half_of + p.slice0 + 5                                # a row the slice's engine reads
    elif p.kind == "QL":
        row = p.NQ + p.NKV + 5                                      # a V row
    else:
        row = 5
    W = p.w[live].astype(F64)
    k1 = int(np.flatnonzero(W[row])[3])
    out = [("one dropped term", R.drop_columns(live, row, k1, 1))]
    for width in (64, 128, 512):
        if width <= K:
            k0 = (K // width - 1) * width if p.kind != "GUa" else 0      # (the sparse gate rows: the chunk that holds the constant)
            out.append((f"a dropped {width}-column k-chunk", R.drop_columns(live, row, k0, width)))
    for rows in (4, 16, 64):
        out.append((f"the last {rows} rows unwritten", R.tail_group(live, rows, False, n_end)))
        out.append((f"the last {rows} rows computed from the last row", R.tail_group(live, rows, True, n_end)))
    out.append(("one fp8 scale block from its neighbour", R.neighbour_scale(live, "fp8", row, 0)))
    out.append(("one NVF4 scale byte from its neighbour", R.neighbour_scale(live, "nvf4", row, k1 // 32 if k1 // 32 + 1 < K // 32 else k1 // 32 - 1)))
    out.append(("two sequences' rows swapped", R.swap_rows(live, 1, 2)))
    slab_w = 128 if K % 128 == 0 else 64
    out.append(("one split-K slab dropped", R.slab(live, K - slab_w, K, -1.0) if p.kind != "GUa" else R.slab(live, 0, slab_w, -1.0)))
    out.append(("one split-K slab added twice", R.slab(live, K - slab_w, K, 1.0) if p.kind != "GUa" else R.slab(live, 0, slab_w, 1.0)))
    # the gamma in front of the live projection; o_proj and down_proj have none: the final norm's, between them and the readout
    out.append(("a gamma shifted by one column", R.gamma_shift(live if p.kind not in ("O", "D") else "lm_head")))
    if p.kind in ("GUa", "GUb"):
        out.append(("gate row n paired with up row n + 1", R.pair_shift()))
    return out


# the narrow shape on both paths; the benchmark's widths where the bars are widest - fp32 activations
@pytest.mark.parametrize("shape,path", [("T", "bf16"), ("T", "f32"), ("W", "f32")])
@pytest.mark.parametrize("kind", R.ALL)
def test_planted_errors_fall_outside_the_bars(kind, shape, path):
    """Each planted error, applied to the float64 oracle of the path: the elements it touches whose reference is below 128 are
    outside the bar (QL: the comparison is exact, every touched element counts), and it touches at least one."""
    p, toks, pos = step_of(kind, shape, sl=R.n_slices(shape) - 1)    # the last slice reads the last rows of I
    c_act, n_bf16, fp32 = PATHS[path]
    want = p.forward(toks, pos, c_act)
    for name, hook in planted(p, toks, pos):
        got = p.forward(toks, pos, c_act, hook=hook)
        over, hit = outside(p, want, got, path, pos), touched(p, want, got)
        if name.startswith("a gamma") and p.kind in ("O", "D"):
            moved = np.roll(p.g_fin, 1) != p.g_fin
            hit = {"logits": np.broadcast_to(moved[None, :], over["logits"].shape) & (np.abs(want["h2"]) > 0.5)}
        n_hit = n_missed = 0
        for key, mask in hit.items():
            if p.kind != "QL":
                mask = mask & (np.abs(want["h2"]) < 128) & (np.abs(got["h2"]) < 128)
            elif key == "logits" and fp32:
                mask = mask & (np.abs(got[key] - want[key]) >= 1.0)   # (a gamma shift also rescales every logit a little)
            n_hit += int(mask.sum())
            n_missed += int((mask & ~over[key]).sum())
        print(f"{kind} {shape} {path}: {name}: {n_hit} elements touched, {n_missed} inside the bars")
        assert n_hit > 0, (kind, shape, path, name, "touches nothing")
        allowed = 0 if name in WHOLE_ROW else n_hit // 10
        assert n_missed <= allowed, (kind, shape, path, name, n_missed, "of", n_hit, "touched elements stay inside the bars")


@pytest.mark.parametrize("shape", SENS_SHAPES)
def test_tie_resolved_to_the_higher_index_is_caught(shape):
    """The planted duplicate: both logits are the same integer, so the token check (lowest index) is what notices."""
    p, toks, pos = step_of("QL", shape)
    f = p.forward(toks, pos, 1.0)
    lo, hi = p.dup
    assert f["logits"][0, lo] == f["logits"][0, hi] == f["logits"][0].max()
    assert int(R.argmax_lowest(f["logits"])[0]) == lo != hi
