"""NumPy restatement of the LSTM forward that lstm_forward / lstm_bidirectional compute (PyTorch's equations and gate order;
the authority is torch.nn.LSTM in float64, recorded in tests/golden/g9_lstm.npz by gen_lstm_golden.py):

    g   = W_ih . x_t + b_ih + b_hh + W_hh . h_{t-1}          gates i, f, g, o in that order along 4H
    c_t = sigmoid(f) * c_{t-1} + sigmoid(i) * tanh(g_g)       h_t = sigmoid(o) * tanh(c_t)

`dtype` is the type every operand, product and sum is held in: float64 (the oracle) or float32 (the yardstick for what fp32
arithmetic alone costs).  `mutate` plants ONE known error, for the test that shows the bars separate right from wrong:
"swap_fg", "swap_io" (two gates exchanged), "no_bhh" (b_hh dropped), "no_h0" / "no_c0" (initial state ignored),
"no_reverse" (reverse=True walks forwards)."""

from __future__ import annotations

import numpy as np

# (B, S, I, H) of the GPU tests, with what each guards (tests/test_lstm_gpu.py); the CPU separation test walks the same list
GPU_SHAPES = ((1, 1, 1, 1), (2, 5, 24, 20), (3, 7, 40, 64), (5, 33, 48, 128), (2, 9, 72, 136), (1, 16, 512, 256), (11, 6, 32, 64))


def case_seed(shape) -> int:
    """The fixed seed of a shape.  The float32 bar is a multiple of max|ref32 - ref64|, and at (1,1,1,1) that maximum is ONE
    sample of a float32 rounding error, which can land arbitrarily close to zero (seed 7152, the formula's value: 1e-9 to 5e-9,
    a thirtieth of half an ulp of 0.5).  Its seed is therefore the first from 7000 on at which the NumPy deviation - of the
    two restatements alone, nothing of the code under test - is at least 3e-8 in the unidirectional, the stateless and both
    bidirectional cases; the other shapes take the formula."""
    B, S, I, H = shape
    if shape == (1, 1, 1, 1):
        return 7048
    return 7000 + 131 * B + 17 * S + 3 * I + H


MUTATIONS = ("swap_fg", "swap_io", "no_bhh", "no_h0", "no_c0", "no_reverse")


def _sigmoid(v):
    return 1 / (1 + np.exp(-v))


def lstm_forward(x, W_ih, W_hh, b_ih, b_hh, h0=None, c0=None, reverse=False, dtype=np.float64, mutate=None):
    """x [B,S,I] -> (output [B,S,H], h_n [B,H], c_n [B,H]); output[:, t] is written at the position processed."""
    if mutate is not None and mutate not in MUTATIONS:
        raise ValueError(f"unknown mutation {mutate!r}")
    x, W_ih, W_hh, b_ih, b_hh = (np.asarray(a, dtype) for a in (x, W_ih, W_hh, b_ih, b_hh))
    B, S, _ = x.shape
    H = W_hh.shape[1]
    h = np.zeros((B, H), dtype) if h0 is None or mutate == "no_h0" else np.asarray(h0, dtype).copy()
    c = np.zeros((B, H), dtype) if c0 is None or mutate == "no_c0" else np.asarray(c0, dtype).copy()
    bias = b_ih if mutate == "no_bhh" else b_ih + b_hh
    order = {"swap_fg": (0, 2, 1, 3), "swap_io": (3, 1, 2, 0)}.get(mutate, (0, 1, 2, 3))
    out = np.zeros((B, S, H), dtype)
    steps = range(S - 1, -1, -1) if reverse and mutate != "no_reverse" else range(S)
    for t in steps:
        g = x[:, t] @ W_ih.T + bias + h @ W_hh.T
        gi, gf, gg, go = (g[:, k * H:(k + 1) * H] for k in order)
        c = _sigmoid(gf) * c + _sigmoid(gi) * np.tanh(gg)
        h = _sigmoid(go) * np.tanh(c)
        out[:, t] = h
    assert out.dtype == dtype and h.dtype == dtype and c.dtype == dtype
    return out, h, c


def lstm_bidirectional(x, W_ih_fwd, W_hh_fwd, b_ih_fwd, b_hh_fwd, W_ih_bwd, W_hh_bwd, b_ih_bwd, b_hh_bwd, dtype=np.float64, mutate=None):
    """-> (output [B,S,2H] forward | backward, h_n [2,B,H], c_n [2,B,H]); zero initial state."""
    of, hf, cf = lstm_forward(x, W_ih_fwd, W_hh_fwd, b_ih_fwd, b_hh_fwd, dtype=dtype, mutate=mutate)
    ob, hb, cb = lstm_forward(x, W_ih_bwd, W_hh_bwd, b_ih_bwd, b_hh_bwd, reverse=True, dtype=dtype, mutate=mutate)
    return np.concatenate([of, ob], axis=2), np.stack([hf, hb]), np.stack([cf, cb])


def make_case(B, S, I, H, seed, state=True):
    """The input distribution of every LSTM test: deliberately large, so the gates leave the linear region."""
    r = np.random.default_rng(seed)
    d = {"x": r.standard_normal((B, S, I)),
         "W_ih": r.uniform(-1, 1, (4 * H, I)) * 2 / np.sqrt(I), "W_hh": r.uniform(-1, 1, (4 * H, H)) * 2 / np.sqrt(H),
         "b_ih": r.uniform(-0.5, 0.5, 4 * H), "b_hh": r.uniform(-0.5, 0.5, 4 * H)}
    if state:
        d["h0"] = r.uniform(-1, 1, (B, H))
        d["c0"] = r.uniform(-2, 2, (B, H))
    return d


WEIGHTS = ("W_ih", "W_hh", "b_ih", "b_hh")


def make_bidir_case(B, S, I, H, seed):
    """x plus one weight set per direction, keyed W_ih_fwd ... b_hh_bwd."""
    f, b = make_case(B, S, I, H, seed, state=False), make_case(B, S, I, H, seed + 1000, state=False)
    d = {"x": f["x"]}
    d.update({f"{k}_fwd": f[k] for k in WEIGHTS})
    d.update({f"{k}_bwd": b[k] for k in WEIGHTS})
    return d


def bidir_args(d):
    return [d["x"]] + [d[f"{k}_fwd"] for k in WEIGHTS] + [d[f"{k}_bwd"] for k in WEIGHTS]
