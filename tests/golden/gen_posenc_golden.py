"""Generate tests/golden/g8_posenc.npz by IMPORTING the reference, as gen_llama4_golden.py does (runs only where the
reference checkout is mounted at /root/reference; needs no GPU, and no test runs it).

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=/root/reference/src:. python3 tests/golden/gen_posenc_golden.py      (from the repository root)

The fixture holds inputs and what the reference's CPU path returns for them: the three rope_init_* tables, the PoPE
encoding and pope_inplace, ALiBi slopes, alibi_compute_bias and alibi_add_bias.  Tables are thinned to the rows `rows_<S>`
(every 7th row up to 100 rows, every 37th and the last beyond) to keep the file at tens of KB."""

from __future__ import annotations

import os

import numpy as np

import pygpukit  # noqa: E402  (the reference, via PYTHONPATH=/root/reference/src)
from pygpukit.core.factory import from_numpy as G  # noqa: E402
from pygpukit.ops.nn import (alibi_add_bias, alibi_compute_bias, alibi_init_slopes, pope_init_encoding, pope_inplace,  # noqa: E402
                             rope_init_linear, rope_init_ntk_aware, rope_init_yarn)

assert "/root/reference" in pygpukit.__file__, pygpukit.__file__

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE_SHAPES = ((64, 16), (70, 40), (300, 128))
SCALES = (1.0, 2.0, 4.0)
YARN_ORIGINAL_MAX_LEN = 64          # all three bands occur at these head dims


def rows(S: int) -> np.ndarray:
    if S <= 16:
        return np.arange(S)
    return np.arange(0, S, 7) if S <= 100 else np.unique(np.append(np.arange(0, S, 37), S - 1))


def thin(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a[rows(a.shape[0])])


def main() -> None:
    out: dict = {"yarn_original_max_len": YARN_ORIGINAL_MAX_LEN}
    for S in (16, 64, 70, 300):
        out[f"rows_{S}"] = rows(S)
    for S, D in TABLE_SHAPES:
        for scale in SCALES:
            tag = f"{S}_{D}_{int(scale)}"
            for name, fn, kw in (("ntk", rope_init_ntk_aware, {}), ("linear", rope_init_linear, {}),
                                 ("yarn", rope_init_yarn, {"original_max_len": YARN_ORIGINAL_MAX_LEN})):
                base = 10000.0 if D != 40 else 500000.0
                cos, sin = fn(S, D, base=base, scale=scale, **kw)
                out[f"{name}_cos_{tag}"], out[f"{name}_sin_{tag}"] = thin(cos.to_numpy()), thin(sin.to_numpy())
    out["pope_enc_16_8"] = pope_init_encoding(16, 8).to_numpy()
    out["pope_enc_300_128"] = thin(pope_init_encoding(300, 128).to_numpy())
    for h in (1, 2, 8, 12, 32, 40):
        out[f"slopes_{h}"] = alibi_init_slopes(h).to_numpy()
    slopes = alibi_init_slopes(8)
    out["bias_5_8_causal"] = alibi_compute_bias(5, 8, slopes, causal=True).to_numpy()
    out["bias_5_8_full"] = alibi_compute_bias(5, 8, slopes, causal=False).to_numpy()

    rng = np.random.default_rng(8001)
    scores = rng.standard_normal((2, 8, 3, 9)).astype(np.float32)
    out["add_bias_scores"] = scores
    g = G(scores.copy())
    alibi_add_bias(g, slopes, start_pos=4)
    out["add_bias_y"] = g.to_numpy()
    assert not np.array_equal(out["add_bias_y"], scores)

    q, k = rng.standard_normal((5, 3, 8)).astype(np.float32), rng.standard_normal((5, 1, 8)).astype(np.float32)
    out["pope_q"], out["pope_k"] = q, k
    gq, gk = G(q.copy()), G(k.copy())
    pope_inplace(gq, gk, pope_init_encoding(16, 8), start_pos=2)
    out["pope_q_y"], out["pope_k_y"] = gq.to_numpy(), gk.to_numpy()
    assert not np.array_equal(out["pope_q_y"], q)

    path = os.path.join(HERE, "g8_posenc.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} entries")
    assert os.path.getsize(path) < 100 * 1024


if __name__ == "__main__":
    main()
