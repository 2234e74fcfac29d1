"""QL probes (tests/engine_linear_ref.py) at vocabularies the GEMV lm_head needs LATER TRIPS for, with planted argmax ties.

The batch-1 / 2 / 4 lm_head is fused_gemv_kernel with 4 rows per wave on a fixed grid of 1024 workgroups: 16 384 rows per
pass.  Wave q of the grid (workgroup q // 4, wave q % 4) owns rows 4 q .. 4 q + 3 of pass 0 and the same rows + 16 384 t of
pass t.  Every vocabulary of the existing exact tests fits one pass; here

    V2 = 16 384 + 16 * 37 + 6     waves 0 .. 149 make two trips, the others one; the last row group holds 2 rows
    V3 = 2 * 16 384 + 16 * 5 + 3  waves 0 .. 20 make three trips, the others two; the last row group holds 3 rows

The probe's arithmetic is the parent module's (integer logits, exact in any order).  On top of it four tokens get an exact
duplicate of their winning lm_head row, both copies at chosen rows (lo, hi), so that the two maximal logits are bit-identical
and only the tie rule decides - the lower row must win:

    "lanes"       rows n0 + 1 and n0 + 3 of one wave and trip (two lanes of one epilogue)
    "waves"       two waves of one workgroup
    "trips"       the first and the second trip of one wave (the lane's running best must keep the earlier row)
    "workgroups"  two workgroups of one pass
NumPy only."""

from __future__ import annotations

import functools

import numpy as np

from tests import engine_linear_ref as R

F32, F64 = np.float32, np.float64
ROWS_PER_WAVE, GRID = 4, 1024
PASS = GRID * 4 * ROWS_PER_WAVE                      # 16 384 rows per pass of the grid
V2 = PASS + 16 * 37 + 6
V3 = 2 * PASS + 16 * 5 + 3
VOCABS = (V2, V3)
# (lo, hi) of every planted tie: wave 53 of workgroup 13 holds rows 212 .. 215; workgroup 40 holds rows 640 .. 655
TIES = {"lanes": (4 * 53 + 1, 4 * 53 + 3), "waves": (16 * 40 + 2, 16 * 40 + 4 * 2 + 1), "trips": (4 * 9 + 2, PASS + 4 * 9 + 2),
        "workgroups": (16 * 100 + 5, 16 * 733 + 5)}
POOL = 96                                            # tokens looked at for unique winners


def trips_of_wave(q: int, vocab: int) -> int:
    return len(range(4 * q, vocab, PASS))


class TailProbe(R.Probe):
    """The QL probe of shape W at a vocabulary beyond one pass: the embedding covers the whole vocabulary (input tokens stay
    below 4096: rows beyond are never read), and the ties of TIES are planted for four tokens."""

    def __init__(self, vocab: int, fmt: str = "bf16"):
        super().__init__("QL", "W", fmt, vocab)
        assert vocab > R.VOCAB and vocab % 4 != 0
        H = self.H
        erng = np.random.default_rng(H)                # the parent's embedding, row for row
        ids = np.arange(R.VOCAB)
        emb = erng.choice(np.array([-1.0, 1.0], F32), size=(R.VOCAB, H))
        emb[:, 0] = 1.0
        emb[:, 1:1 + R.NBITS] = np.where((ids[:, None] >> np.arange(R.NBITS)[None, :]) & 1, 1.0, -1.0)
        full = np.ones((vocab, H), F32)
        full[:R.VOCAB] = emb
        self.emb = full
        lm = self.lm.copy()
        x = emb[:POOL] * self.g_fin                    # the final norm's output for tokens 0 .. POOL - 1: integers
        taken = set(self.dup)
        self.ties = {}
        t = 0
        for name, (lo, hi) in TIES.items():
            assert lo < hi < vocab and not {lo, hi} & taken
            while True:                                # the next token with a single winning row clear of every planted row
                m = x[t] @ lm.T
                win = int(np.argmax(m))
                if t != self.dup_token and np.count_nonzero(m == m[win]) == 1 and win not in taken | {lo, hi}:
                    break
                t += 1
            lm[[lo, win]] = lm[[win, lo]]              # the winner moves to lo ...
            lm[hi] = lm[lo]                            # ... and its copy to hi
            taken |= {lo, hi, win}
            self.ties[name] = (t, lo, hi)
            t += 1
        m = x @ lm.T                                   # [POOL, vocab] float32: integer sums, exact
        top = m.max(axis=1, keepdims=True)
        n_top = (m == top).sum(axis=1)
        for name, (tok, lo, hi) in self.ties.items():
            assert n_top[tok] == 2 and m[tok, lo] == m[tok, hi] == top[tok, 0], name
        tied = {tok for tok, _, _ in self.ties.values()}
        self.unique = tuple(int(i) for i in np.flatnonzero(n_top == 1) if i not in tied and i != self.dup_token)
        lm.setflags(write=False)
        full.setflags(write=False)
        self.lm = lm

    def tokens(self, batch: int, first: str | None = None) -> list[int]:
        """Distinct tokens of a step: unique winners, sequence 0 the tie `first` when one is named."""
        toks = [self.unique[(7 * s + 3) % len(self.unique)] for s in range(batch)]
        if first is not None:
            toks[0] = self.ties[first][0]
        assert len(set(toks)) == batch
        return toks


@functools.lru_cache(maxsize=None)
def tail_probe(vocab: int, fmt: str = "bf16") -> TailProbe:
    return TailProbe(vocab, fmt)


# ---- planted errors: what the lm_head of a broken trip loop would return (hooks for Probe.forward) ----------------------------
def dropped_trip(t: int):
    """Pass t's rows never written (the logits buffer keeps zeros)."""
    def fn(W, X, Y):
        Y[:, t * PASS:(t + 1) * PASS] = 0.0
        return Y
    return R.on("lm_head", fn)


def reread_first_trip(t: int):
    """Pass t computed from pass 0's rows (the next trip's row base not advanced)."""
    def fn(W, X, Y):
        n = Y[:, t * PASS:(t + 1) * PASS].shape[1]
        Y[:, t * PASS:t * PASS + n] = Y[:, :n]
        return Y
    return R.on("lm_head", fn)


def stale_last_group():
    """The partial last row group computed from the last row alone (the clamp applied to every row of the group)."""
    def fn(W, X, Y):
        n = Y.shape[1] % ROWS_PER_WAVE
        Y[:, -n:] = Y[:, -1:]
        return Y
    return R.on("lm_head", fn)


def argmax_highest(logits: np.ndarray) -> np.ndarray:
    """A tie resolved to the HIGHER index."""
    return logits.shape[-1] - 1 - np.argmax(logits[..., ::-1], axis=-1)
