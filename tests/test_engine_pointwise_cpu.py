"""tests/engine_pointwise_ref.py without a device: the probe oracle against the project's oracle, a float32 restatement with
the table's roundings against every bar, the planted errors against every readout that claims them (each must leave the bar by
4x on at least one element - a condition on the data, asserted), and the branch tables of the GPU cases."""

from __future__ import annotations

import numpy as np
import pytest

from oracle import cpu_ref as O
from tests import engine_pointwise_ref as R

F32, F64 = np.float32, np.float64
KIND_SHAPES = [("NR", "W"), ("NR", "T"), ("NR", "X"), ("NR", "P"), ("NR", "H5"), ("NRo", "W"), ("NRo", "T"), ("NRo", "X"), ("NRo", "P"), ("S", "W"), ("S", "T")]
PATHS = {"f32": R.Path(0, False, 0, 0), "bf16": R.Path(1, False, 1, 1), "carried": R.Path(1, True, 1, 1), "fp8a8": R.Path(1, False, 1, 1, True)}
WIDEST = R.Path(1, True, 1, 1)                       # (and 16 slab additions, the most any path has)


def cases(kind: str):
    """(tokens, positions) of a decode step and of a prompt, as the GPU test runs them."""
    yield R.decode_tokens(kind, 19), R.decode_positions(kind, 19)
    if kind == "NRo":
        yield R.prompt_tokens(1), [0]
    else:
        yield R.prompt_tokens(33), list(range(33))
        yield R.prompt_tokens(20, 100), list(range(100, 120))


def project_oracle(p, toks, pos):
    """oracle.cpu_ref.build_qwen3_ref on the probe's weights, in float64: (final hidden, K, V, logits)."""
    w = {k: v.astype(F64) for k, v in p.w.items()}
    lw = dict(q=w["w_qkv"][:p.QD], k=w["w_qkv"][p.QD:p.QD + p.NKV], v=w["w_qkv"][p.QD + p.NKV:], o=w["w_o"], gate=w["w_gate_up"][:p.I],
              up=w["w_gate_up"][p.I:], down=w["w_down"], attn_norm=p.g_attn.astype(F64), mlp_norm=p.g_mlp.astype(F64))
    if p.qk_norm:
        lw.update(q_norm=p.g_q.astype(F64), k_norm=p.g_k.astype(F64))
    layers = [lw]
    if p.L == 2:      # the pass-through layer in front: zero matrices, gammas of its own
        ga, gm, gq, gk = (g.astype(F64) for g in p.pass_gammas)
        layers.insert(0, {**{k: np.zeros_like(v) for k, v in lw.items() if v.ndim == 2}, "attn_norm": ga, "mlp_norm": gm, "q_norm": gq, "k_norm": gk})
    model = O.build_qwen3_ref(p.cfg, {"embed": p.emb.astype(F64), "layers": layers, "final_norm": p.g_fin.astype(F64), "lm_head": p.lm.astype(F64)},
                              max_pos=max(pos) + 1)
    hid, K, V = [], [], []
    for t, q in zip(toks, pos):                                   # row by row: the probe's attention is own-row
        h, pres = model([t], position_ids=[q], use_cache=True)
        hid.append(h[0]); K.append(pres[-1][0][0]); V.append(pres[-1][1][0])
    hid = np.stack(hid)
    return hid, np.stack(K), np.stack(V), model.get_logits(hid)


@pytest.mark.parametrize("kind,shape,qk_norm,layers", [(k, s, True, 1) for k, s in KIND_SHAPES]
                         + [("NR", "W", False, 1), ("NR", "T", False, 1), ("NR", "W", True, 2)])
def test_probe_oracle_is_the_project_oracle(kind, shape, qk_norm, layers):
    """Hidden state, K, V and logits of Probe.forward equal build_qwen3_ref's on the same weights to float64 round-off; K also
    carries the two tables' difference - the project oracle takes cos / sin in float32, the engine in double rounded to
    float32: one float32 ulp of each, 2 u (|k1| + |k2|).  Every slice's probe, every row of the decode case and a prompt's
    first rows; the fp8 and NVF4 probes hold the same arrays (their encoders assert exactness), so bf16 stands for them."""
    for sl in R.slices(kind, shape):
        _oracle_case(R.probe(kind, shape, sl=sl, qk_norm=qk_norm, layers=layers), kind)


def _oracle_case(p, kind):
    toks, pos = (a + b for a, b in zip(next(cases(kind)), (R.prompt_tokens(6, 100), list(range(100, 106))) if kind != "NRo" else ([], [])))
    f = p.forward(toks, pos)
    hid, K, V, logits = project_oracle(p, toks, pos)
    tol = 1e-11
    assert np.abs(hid - f["xf"]).max() <= tol * np.abs(f["xf"]).max()
    assert (np.abs(V - f["v"]) <= tol * np.abs(f["v"]) + 1e-300).all()
    # (NRo: x + o may cancel, so round-off is measured against the row's largest element)
    assert (np.abs(logits[:, :p.H] - f["logits"]) <= tol * np.abs(f["logits"]).max(1, keepdims=True) + 1e-300).all() and not logits[:, p.H:].any()
    half = p.D // 2
    k12 = np.abs(f["kn"][..., :half]) + np.abs(f["kn"][..., half:])
    assert (np.abs(K - f["k"]) <= 2 * R.U * np.concatenate([k12, k12], -1) + tol * np.abs(f["k"]) + 1e-300).all()


@pytest.mark.parametrize("kind,shape,path", [(k, s, pa) for k, s in KIND_SHAPES for pa in PATHS if not (pa == "fp8a8" and k == "NRo")])
def test_float32_restatement_stays_inside_the_bars(kind, shape, path):
    """float32 arithmetic with the bf16 roundings where the table puts them (x^ fp32 or bf16; the carried order
    bf16(h gamma) inv; act and the final x^ rounded or not; x^ and act through the e4m3 row quantiser on the fp8 x fp8 prefill,
    which has no NRo case) stays inside every bar of its path."""
    pa = PATHS[path]
    for sl in R.slices(kind, shape):
        p = R.probe(kind, shape, sl=sl)
        for toks, pos in cases(kind):
            f = p.forward(toks, pos)
            e = p.forward(toks, pos, T=F32, path=pa)
            assert (np.abs(e["v"] - f["v"]) <= p.v_bar(f, pa)).all()
            over = np.abs(e["k"] - f["k"]) / p.k_bar(f, pa, pos)
            assert over.max() <= 1.0, (kind, shape, path, float(over.max()))
            if kind == "S":
                over = np.abs(p.ratio(e["logits"].astype(F64), toks) - f["h2"][:, p.half:]) / p.s_bar(f, pa)
            else:
                over = np.abs(e["logits"] - f["logits"]) / p.logit_bar(f, pa)
            assert over.max() <= 1.0, (kind, shape, path, float(over.max()))


def exceed(p, kind, mut, readout, cases_, WIDEST=WIDEST):
    """The largest |mutated - oracle| / bar over the elements of `readout`, on the widest path's bar."""
    worst = 0.0
    for toks, pos in cases_:
        f, m = p.forward(toks, pos), p.forward(toks, pos, mut=mut)
        if readout == "V":
            r = np.abs(m["v"] - f["v"]) / p.v_bar(f, WIDEST)
        elif readout == "K":
            r = np.abs(m["k"] - f["k"]) / p.k_bar(f, WIDEST, pos)
        elif readout == "S":
            r = np.abs(p.ratio(m["logits"], toks) - f["h2"][:, p.half:]) / p.s_bar(f, WIDEST)
        else:
            r = np.abs(m["logits"] - f["logits"]) / p.logit_bar(f, WIDEST)
        worst = max(worst, float(r.max()))
    return worst


PLANTED = [(kind, shape, readout, mut)
           for kind, shape, readouts in ([("NR", sh, ("V", "logits", "K")) for sh in ("W", "T", "X", "P", "H5")]
                                         + [("NRo", sh, ("logits", "o")) for sh in ("W", "T", "X", "P")] + [("S", "W", ("S",)), ("S", "T", ("S",))])
           for readout in readouts for mut in R.MUTATIONS[readout]]
PLANTED += [("NR", "H5", "V", "sum_4096"), ("NR", "H5", "logits", "sum_4096")]


@pytest.mark.parametrize("kind,shape,readout,mut", PLANTED)
def test_planted_error_leaves_the_bar(kind, shape, readout, mut):
    """On EVERY slice's probe (the weight formats share the bf16 probe's arrays, so it stands for fp8 and NVF4)."""
    for sl in R.slices(kind, shape):
        worst = exceed(R.probe(kind, shape, sl=sl), kind, mut, "logits" if readout == "o" else readout, list(cases(kind)))
        assert worst >= 4.0, (kind, shape, sl, readout, mut, worst)


# the fp8 x fp8 prefill's bars carry half an e4m3 spacing (2**-4 relative): "mean over H - 128 columns" (a 6 % shift of g) and
# gelu for silu are NOT claimed at its S readout; everything else is
A8_PLANTED = [("NR", ro, mut) for ro in ("V", "K") for mut in R.MUTATIONS[ro]] + [("S", "S", mut) for mut in R.MUTATIONS["S"] if mut not in ("mean_h128", "gelu")]


@pytest.mark.parametrize("kind,readout,mut", A8_PLANTED)
def test_planted_error_leaves_the_fp8a8_bar(kind, readout, mut):
    case = [(R.prompt_tokens(129), list(range(129)))]
    worst = exceed(R.probe(kind, "W", "fp8a8"), kind, mut, readout, case, PATHS["fp8a8"])
    assert worst >= 4.0, (kind, readout, mut, worst)


def test_carried_attn_norm_of_the_two_layer_probe():
    """The W-2layer rig: the float32 restatement of the carried order stays inside the (wider) V and K bars, and the planted
    errors of both readouts still leave them by 4x."""
    p = R.probe("NR", "W", layers=2)
    pa = PATHS["carried"]
    for toks, pos in cases("NR"):
        f, e = p.forward(toks, pos), p.forward(toks, pos, T=F32, path=pa)
        assert (np.abs(e["v"] - f["v"]) <= p.v_bar(f, pa)).all() and (np.abs(e["k"] - f["k"]) <= p.k_bar(f, pa, pos)).all()
        assert (np.abs(e["logits"] - f["logits"]) <= p.logit_bar(f, pa)).all()
    for ro in ("V", "K"):
        for mut in R.MUTATIONS[ro]:
            assert exceed(p, "NR", mut, ro, list(cases("NR")), pa) >= 4.0, (ro, mut)


def q_cases(p, B):
    """The Q probe's steps at batch B with the cache rows a bf16 device path would hold (the float32 restatement of NR)."""
    for k in range(R.q_steps(p, B)):
        toks, pos, prompts = R.q_case(p, B, k)
        K, V = [], []
        for t, n, pr in zip(toks, pos, prompts):
            ff = p.forward(pr + [t], list(range(n + 1)), T=F32, path=PATHS["bf16"])
            K.append(ff["k"].astype(F64)); V.append(ff["v"].astype(F64))
        yield toks, pos, K, V


@pytest.mark.parametrize("shape,fmt", [("W", "bf16"), ("T", "bf16"), ("X", "bf16"), ("P", "bf16"), ("W", "fp8"), ("W", "nvf4")])
def test_q_readout(shape, fmt):
    """A float32 restatement (bf16 x^, q, probabilities and attention output) stays inside the Q bar, on fp32 and bf16 chunks;
    every planted error of Q_MUTATIONS leaves it by 4x on some element; scores are of order 1 (no saturated softmax)."""
    p = R.probe("Q", shape, fmt)
    worst = dict.fromkeys(R.Q_MUTATIONS, 0.0)
    for B in (1, 5):
        for toks, pos, K, V in q_cases(p, B):
            for act_bf16 in (False, True):
                f = p.q_forward(toks, pos, K, V, act_bf16, True)
                e = p.q_forward(toks, pos, K, V, act_bf16, True, emulate=True)
                assert (np.abs(e["logits"] - f["logits"]) <= f["bar"]).all()
            assert np.abs(f["q"]).max() < 1.0
            for mut in R.Q_MUTATIONS:
                m = p.q_forward(toks, pos, K, V, True, True, mut=mut)
                worst[mut] = max(worst[mut], float((np.abs(m["logits"] - f["logits"]) / f["bar"]).max()))
    assert min(worst.values()) >= 4.0, worst


def test_table_row_clamped_one_early_leaves_the_bar():
    """Seen only on the last row of the cache: the max_batch-1 engine with a 4096-row cache decodes at position 4095."""
    p = R.probe("NR", R.LONG["shape"], max_seq=R.LONG_CACHE)
    pos = [R.LONG["pos"]]
    f, m = p.forward([20], pos), p.forward([20], pos, mut="clamp_early")
    assert (np.abs(m["k"] - f["k"]) / p.k_bar(f, WIDEST, pos)).max() >= 4.0


def test_qk_gamma_exchange_needs_qk_norm():
    """q_norm != k_norm, element by element: an exchange moves every K element."""
    p = R.probe("NR", "W")
    assert (p.g_q != p.g_k).all() and not np.array_equal(p.g_attn, p.g_mlp) and not np.array_equal(p.g_mlp, p.g_fin)


def test_probe_data_meet_the_issue():
    """rms 2**-6 .. 2**6 across tokens, an outlier row, a constant row, a row at eps, a row far below; gates at 0, +-small, either
    side of -88.7 and beyond 17."""
    p = R.probe("NR", "W")
    ms = (p.emb.astype(F64) ** 2).mean(1)
    gen = np.flatnonzero(~np.isin(np.arange(p.V) % 16, (3, 5, 7, 9)))
    assert np.sqrt(ms[gen]).min() < 2.0 ** -5.5 and np.sqrt(ms[gen]).max() > 2.0 ** 5.5
    assert 0.3 < ms[7] / R.EPS < 3.0 and ms[9] < 1e-4 * R.EPS
    assert np.unique(p.emb[5]).size == 1
    row = np.abs(p.emb[3].astype(F64))
    assert row.max() >= 2.0 ** 9 * np.median(row)
    s = R.probe("S", "W")
    toks = R.decode_tokens("S", 19)
    g = s.forward(toks, [0] * 19)["g"]
    assert (g == 0).any() and (np.abs(g[g != 0]) < 0.05).any() and (g < -88.8).any() and ((g > -88.6) & (g < -40)).any() and (g > 17).any()
    assert g.min() > -400 and g.max() < 60
    for fmt in ("fp8", "nvf4"):                                     # every matrix is exact in the quantised formats (the encoders assert it)
        R.probe("S", "W", fmt)
        R.probe("NRo", "W", fmt)


def test_every_case_names_its_branch():
    for rid, cfg in R.RIGS.items():
        for B in cfg["decode"]:
            assert (rid, B) in R.EXPECT, (rid, B)
        lengths = set(cfg["prefill"]) | (set(R.CHUNKED) if cfg["chunked"] else set())
        if "NRo" in cfg["kinds"] and cfg["prefill"]:
            lengths.add(1)
        for n in lengths:
            assert (rid, n) in R.PREFILL_EXPECT, (rid, n)
        assert set(cfg["replay"]) <= set(cfg["decode"])
    for rid, batches in R.Q_RIGS.items():
        assert all((rid, B) in R.EXPECT for B in batches), rid
