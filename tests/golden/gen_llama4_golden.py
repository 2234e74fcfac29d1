"""Generate tests/golden/g7_llama4.npz by IMPORTING the reference, as gen_golden.py does (runs only where the
reference checkout is mounted at /root/reference; needs no GPU, and no test runs it).

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=/root/reference/src:. python3 tests/golden/gen_llama4_golden.py      (from the repository root)

The fixture holds inputs and what the reference's CPU path returns for them: l2norm, irope_scale_q, sdpa_irope, and a
two-layer Llama4Model (prefill logits of a 12-token prompt, 6 greedy tokens).  The model's weights are not stored: they
are re-drawn from the seed with tests.llama4_ref.make_llama4_weights, and only their checksum is kept."""

from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))

from tests import llama4_ref as R  # noqa: E402  (weight generator and shapes only)

import pygpukit  # noqa: E402  (the reference, via PYTHONPATH=/root/reference/src)
from pygpukit.core.factory import from_numpy as G  # noqa: E402
from pygpukit.llm.models import llama4 as L  # noqa: E402
from pygpukit.ops.nn import irope_scale_q, l2norm, sdpa_irope  # noqa: E402

assert "/root/reference" in pygpukit.__file__, pygpukit.__file__

PROMPT_LEN, NEW_TOKENS, GAP = 12, 6, 5e-2


def gen_ops(out: dict) -> None:
    rng = np.random.default_rng(7001)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    x = f(6, 128)
    out["l2norm_a_x"], out["l2norm_a_eps"], out["l2norm_a_y"] = x, 1e-6, l2norm(G(x)).to_numpy()
    x = f(3, 5, 40)
    out["l2norm_b_x"], out["l2norm_b_eps"], out["l2norm_b_y"] = x, 1e-5, l2norm(G(x), eps=1e-5).to_numpy()

    q, pos = f(9, 2, 8), np.arange(9, dtype=np.int64)
    out["scale_q_q"], out["scale_q_pos"], out["scale_q_params"] = q, pos, np.array([0.5, 2.0])
    out["scale_q_y"] = irope_scale_q(G(q), G(pos), attn_scale=0.5, floor_scale=2.0).to_numpy()

    for tag, (hq, hkv, ql, kvl, d), off, p0 in (("a", (4, 2, 40, 40, 64), 0, 0), ("b", (2, 2, 12, 30, 128), 18, 18)):
        q, k, v = f(hq, ql, d), f(hkv, kvl, d), f(hkv, kvl, d)
        pos = np.arange(p0, p0 + ql, dtype=np.int64)
        out[f"sdpa_{tag}_q"], out[f"sdpa_{tag}_k"], out[f"sdpa_{tag}_v"], out[f"sdpa_{tag}_pos"] = q, k, v, pos
        out[f"sdpa_{tag}_params"] = np.array([0.5, 16.0, off])
        out[f"sdpa_{tag}_y"] = sdpa_irope(G(q), G(k), G(v), G(pos), attn_scale=0.5, floor_scale=16.0, causal_offset=off).to_numpy()


def reference_model(cfg: dict, w: dict) -> "L.Llama4Model":
    """The reference multiplies x @ W with W [in, out]: hand it the transposes, as its own loader does."""
    c = L.Llama4Config(max_position_embeddings=4096, no_rope_layers=None, **cfg)
    t = lambda a: G(np.ascontiguousarray(a.T))  # noqa: E731
    blocks = []
    for lw in w["layers"]:
        attn = L.Llama4Attention(t(lw["q"]), t(lw["k"]), t(lw["v"]), t(lw["o"]), c)
        blocks.append(L.Llama4Block(attn, L.Llama4MLP(t(lw["gate"]), t(lw["up"]), t(lw["down"])), G(lw["input_norm"]), G(lw["post_norm"]),
                                    c.rms_norm_eps))
    return L.Llama4Model(c, G(w["embed"]), blocks, G(w["norm"]), t(w["lm_head"]))


def gen_model(out: dict) -> None:
    cfg = R.TINY_CFG
    for seed in range(100):
        w = R.make_llama4_weights(cfg, seed)
        model = reference_model(cfg, w)
        prompt = np.random.default_rng(900 + seed).integers(0, cfg["vocab_size"], PROMPT_LEN).astype(np.int64)
        ids, gaps = list(prompt), []
        for _ in range(NEW_TOKENS):
            last = model.forward(np.array(ids, np.int64)).to_numpy()[-1].astype(np.float64)
            top = np.sort(last)
            gaps.append((top[-1] - top[-2]) / np.abs(last).max())
            ids.append(int(np.argmax(last)))
        print(f"seed {seed}: smallest top-1/top-2 gap {min(gaps):.3f} of max|logit|")
        if min(gaps) >= GAP:
            break
    assert min(gaps) >= GAP, "no seed with a safe greedy margin"
    tokens = L.generate(model, prompt, max_new_tokens=NEW_TOKENS, eos_token_id=-1)
    assert list(tokens) == ids
    out["model_seed"], out["model_prompt"], out["model_min_gap"] = seed, prompt, min(gaps)
    out["model_logits"] = model.forward(prompt).to_numpy().astype(np.float32)
    out["model_tokens"] = np.array(ids[PROMPT_LEN:], np.int64)
    out["model_weight_checksum"] = R.checksum(w)


def main() -> None:
    out: dict = {}
    gen_ops(out)
    gen_model(out)
    path = os.path.join(HERE, "g7_llama4.npz")
    np.savez(path, **out)
    size = os.path.getsize(path)
    limit = max(os.path.getsize(os.path.join(HERE, n)) for n in os.listdir(HERE) if n.endswith(".npz") and n != "g7_llama4.npz")
    print(f"wrote {path}: {size} bytes, {len(out)} entries")
    assert size <= limit, (size, limit)


if __name__ == "__main__":
    main()
