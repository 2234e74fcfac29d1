"""NumPy side of tests/test_gpu_gemv_tail.py: the probes' preconditions at the multi-trip vocabularies, the planted ties, and
the planted errors - each must leave the bar the GPU test applies, or the token check, before a GPU ever sees the probe."""

from __future__ import annotations

import numpy as np
import pytest

from tests import engine_linear_ref as R
from tests import gemv_tail_ref as T

BATCHES = (1, 2, 4)


@pytest.fixture(scope="module", params=T.VOCABS)
def probe(request):
    return T.tail_probe(request.param)


def test_vocabularies_take_the_trips_the_tests_name():
    assert T.V2 % 4 == 2 and T.V3 % 4 == 3                       # a partial last row group of 2 and of 3 rows
    waves = T.GRID * 4
    assert {T.trips_of_wave(q, T.V2) for q in range(waves)} == {1, 2} and {T.trips_of_wave(q, T.V3) for q in range(waves)} == {2, 3}
    for lo, hi in T.TIES.values():
        assert lo < hi < min(T.VOCABS)
    lo, hi = T.TIES["lanes"]
    assert lo // 4 == hi // 4 and (lo % 4, hi % 4) == (1, 3)
    lo, hi = T.TIES["waves"]
    assert lo // 16 == hi // 16 and lo // 4 != hi // 4
    lo, hi = T.TIES["trips"]
    assert hi - lo == T.PASS and lo < T.PASS
    lo, hi = T.TIES["workgroups"]
    assert lo // 16 != hi // 16 and hi < T.PASS


def test_preconditions(probe):
    """Integer-exact sums inside the probe's limits for every step the GPU test decodes; unique winners except the planted ties."""
    p = probe
    steps = [p.tokens(b) for b in BATCHES] + [p.tokens(b, first=tie) for tie in T.TIES for b in (1, 4)]
    for toks in steps:
        pos = R.decode_positions("QL", len(toks))
        f = p.forward(toks, pos, 1.0)
        p.check_conditions(toks, pos, f=f, fc=p.forward(toks, pos, R.C64))
        logits = f["logits"]
        top = logits.max(axis=1)
        for s, t in enumerate(toks):
            at = np.flatnonzero(logits[s] == top[s])
            tied = [v for v in p.ties.values() if v[0] == t]
            if tied:
                assert at.tolist() == [tied[0][1], tied[0][2]], (t, at)
            else:
                assert len(at) == 1, (t, at)
                # the margin to the runner-up is an integer: wider than any fp32 accumulation bar
                assert top[s] - np.partition(logits[s], -2)[-2] >= 1.0
    assert len({v[0] for v in p.ties.values()}) == len(T.TIES) and len(p.unique) >= 8


def _leaves_the_bar(p, toks, hook) -> bool:
    pos = R.decode_positions("QL", len(toks))
    out = []
    for c_act, fp32 in ((R.C64, True), (1.0, False)):              # GEMV chunks of 1 and 2 sequences; of 4
        f, bad = p.forward(toks, pos, c_act), p.forward(toks, pos, c_act, hook=hook)
        bar = p.ql_logit_bar(f) if fp32 else np.zeros_like(f["logits"])
        out.append(bool((np.abs(bad["logits"] - f["logits"]) > bar).any()))
    return all(out)


def test_planted_errors_leave_the_bar(probe):
    p = probe
    toks = p.tokens(4)
    trips = -(-p.V // T.PASS)
    for t in range(1, trips):
        assert _leaves_the_bar(p, toks, T.dropped_trip(t)), ("dropped trip", t)
        assert _leaves_the_bar(p, toks, T.reread_first_trip(t)), ("re-read first trip", t)
    assert _leaves_the_bar(p, toks, T.stale_last_group())
    assert not _leaves_the_bar(p, toks, None)


def test_a_tie_resolved_upwards_fails_the_token_check(probe):
    p = probe
    for tie, (tok, lo, hi) in p.ties.items():
        toks = p.tokens(4, first=tie)
        logits = p.forward(toks, R.decode_positions("QL", 4), 1.0)["logits"]
        assert R.argmax_lowest(logits)[0] == lo and T.argmax_highest(logits)[0] == hi
        assert np.array_equal(R.argmax_lowest(logits)[1:], T.argmax_highest(logits)[1:])
