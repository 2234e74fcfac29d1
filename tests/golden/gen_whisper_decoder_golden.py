"""Records tests/golden/g11_whisper_decoder.npz from the reference package's own CPU path (its CPU backend: no GPU, float32).

    python tests/golden/gen_whisper_decoder_golden.py <path to the reference's src directory> [--search FIRST LAST]

Only this generator imports the reference (`pygpukit`); the tests read the fixture.  Recorded, on
tests/whisper_decoder_ref.py's fixture_config() with weights make_decoder_weights(cfg, seed) (untied proj_out, k_proj biases None)
and encoder states make_encoder_states(cfg, 37, seed + 1):
  * seed, enc, ids, logits: the reference WhisperDecoder's logits [1, 5, 203] of the fixed sequence FIXTURE_IDS;
  * tokens: its generate(enc, max_length=20, temperature=0.0).

Conditions asserted on the recorded run (a seed that misses one is not recorded):
  * no EOS before 20 tokens, at least 10 distinct tokens;
  * the smallest top-1 / top-2 logit gap over the 19 generated steps is >= 5e-3 of the largest |logit|, so float32 arithmetic in
    another summation order cannot change a token;
  * for the 16-bit GPU tests, which compare tokens up to the first step whose gap is below 4x their measured logit error and
    need 8 such steps: the NumPy oracle on bf16- and on f16-rounded weights has a gap >= 3e-2 of the largest |logit| on each
    of its first 10 steps (a bf16 logit carries 2^-9 of its magnitude in rounding alone).
`--search` prints those figures from the NumPy oracle for a range of seeds (no reference needed for that part); of seeds 1..400 nine
meet all of them; 156 has the widest 16-bit margin (7.6e-2) and is the one recorded."""

from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
from tests import whisper_decoder_ref as R  # noqa: E402

GAP32, GAP16, STEPS16 = 5e-3, 3e-2, 10


def oracle_figures(seed: int) -> dict:
    cfg = R.fixture_config()
    tensors = R.make_decoder_weights(cfg, seed)
    enc = R.make_encoder_states(cfg, R.FIXTURE_ENC_ROWS, seed + 1)[0]
    out = {}
    for rd in ("f32", "bf16", "f16"):
        tokens, rows = R.DecoderRef(cfg, tensors, np.float64, rd).generate(enc, R.FIXTURE_STEPS, return_logits=True)
        gaps = np.array([R.top2_gap(r) for r in rows]) / np.abs(rows).max()
        out[rd] = (tokens, gaps)
    return out


def meets(fig: dict) -> bool:
    cfg = R.fixture_config()
    tokens, gaps = fig["f32"]
    ok = len(tokens) == R.FIXTURE_STEPS and cfg.eos_token_id not in tokens and len(set(tokens)) >= 10 and gaps.min() >= GAP32
    return ok and all(len(fig[rd][1]) >= STEPS16 and fig[rd][1][:STEPS16].min() >= GAP16 for rd in ("bf16", "f16"))


def search(first: int, last: int) -> None:
    for seed in range(first, last + 1):
        fig = oracle_figures(seed)
        tokens, gaps = fig["f32"]
        print(seed, "ok" if meets(fig) else "--", "distinct", len(set(tokens)), "len", len(tokens), "min gap f32 %.4f" % gaps.min(),
              " ".join("%s first-%d %.4f" % (rd, STEPS16, fig[rd][1][:STEPS16].min()) for rd in ("bf16", "f16")))


def main(ref_src: str) -> None:
    sys.path.insert(0, ref_src)
    from pygpukit.asr.whisper.config import WhisperConfig as RefConfig
    from pygpukit.asr.whisper.decoder import WhisperDecoder as RefDecoder
    from pygpukit.asr.whisper.loader import WhisperWeights as RefWeights
    from pygpukit.core import from_numpy

    seed = R.FIXTURE_SEED
    cfg = R.fixture_config()
    rcfg = RefConfig.from_dict(cfg.to_dict())
    tensors = R.make_decoder_weights(cfg, seed)
    rw = RefWeights(rcfg)
    rw._load_decoder_weights(tensors)
    assert rw.decoder_layers[0]["self_attn_k_bias"] is None and rw.decoder_layers[0]["cross_attn_k_bias"] is None
    assert rw.proj_out_weight is not rw.decoder_embed_tokens and len(rw.decoder_layers[0]) == 26
    enc = R.make_encoder_states(cfg, R.FIXTURE_ENC_ROWS, seed + 1)
    dec = RefDecoder(rcfg, rw)
    ids = np.array([R.FIXTURE_IDS], dtype=np.int64)
    logits = dec(from_numpy(ids), from_numpy(enc)).to_numpy()
    assert logits.shape == (1, len(R.FIXTURE_IDS), cfg.vocab_size) and logits.dtype == np.float32
    tokens = [int(t) for t in dec.generate(from_numpy(enc), max_length=R.FIXTURE_STEPS, temperature=0.0)]

    # the conditions, on the reference's own run: its logits along the generated sequence give the gaps
    assert len(tokens) == R.FIXTURE_STEPS and cfg.eos_token_id not in tokens, tokens
    assert len(set(tokens)) >= 10, tokens
    along = dec(from_numpy(np.array([tokens[:-1]], dtype=np.int64)), from_numpy(enc)).to_numpy()[0]
    assert [int(np.argmax(r)) for r in along] == tokens[1:]
    gap = min(R.top2_gap(r) for r in along) / float(np.abs(along).max())
    assert gap >= GAP32, gap
    fig = oracle_figures(seed)
    assert meets(fig) and fig["f32"][0] == tokens, (fig, tokens)

    path = os.path.join(HERE, "g11_whisper_decoder.npz")
    np.savez_compressed(path, seed=np.array(seed), enc=enc, ids=ids, logits=logits, tokens=np.array(tokens, dtype=np.int64))
    print("seed", seed, "tokens", tokens, "min gap / max |logit| %.4f" % gap, "max |logit| %.3f" % float(np.abs(along).max()),
          os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) >= 5 and sys.argv[2] == "--search":
        search(int(sys.argv[3]), int(sys.argv[4]))
    else:
        main(sys.argv[1])
