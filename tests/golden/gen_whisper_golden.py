"""Records tests/golden/g10_whisper.npz from the reference package's own CPU path (its CPU backend: no GPU, float32).

    python tests/golden/gen_whisper_golden.py <path to the reference's src directory>

Only this generator imports the reference (`pygpukit`); the tests read the fixture.  Recorded:
  * enc_mel, enc_seed, enc_out: the reference WhisperEncoder on tests/whisper_ref.py's fixture_config(), weights from
    make_weights(cfg, enc_seed) (k_proj bias None), mel [1, 16, 74] -> (1, 37, 128);
  * c{i}_x / c{i}_w / c{i}_b / c{i}_out: the reference conv1d (its im2col CPU path) on the cases of FIXTURE_CONV;
  * a_q / a_k / a_v / a_out: one attention through batched_matmul -> * scale -> softmax -> batched_matmul, as the reference
    encoder runs it, with q_len != kv_len."""

from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
from tests import whisper_ref as R  # noqa: E402


def main(ref_src: str) -> None:
    sys.path.insert(0, ref_src)
    from pygpukit.asr.whisper.config import WhisperConfig as RefConfig
    from pygpukit.asr.whisper.encoder import WhisperEncoder as RefEncoder
    from pygpukit.asr.whisper.loader import WhisperWeights as RefWeights
    from pygpukit.core import from_numpy
    from pygpukit.ops.conv import conv1d
    from pygpukit.ops.matmul import batched_matmul
    from pygpukit.ops.reduction import softmax

    rec = {}
    cfg = R.fixture_config()
    rcfg = RefConfig.from_dict(cfg.to_dict())
    tensors = R.make_weights(cfg, R.FIXTURE_SEED)
    rw = RefWeights(rcfg)
    rw._load_encoder_weights(tensors)
    assert rw.encoder_layers[0]["self_attn_k_bias"] is None
    mel = R.make_mel(cfg, R.FIXTURE_FRAMES, R.FIXTURE_SEED + 1)
    out = RefEncoder(rcfg, rw)(from_numpy(mel)).to_numpy()
    assert out.shape == (1, cfg.max_source_positions, cfg.d_model) and out.dtype == np.float32
    rec.update(enc_mel=mel, enc_seed=np.array(R.FIXTURE_SEED), enc_out=out)

    for i, case in enumerate(R.FIXTURE_CONV):
        x, w, b = R.make_conv_case(case, bias=i != 3)
        y = conv1d(from_numpy(x), from_numpy(w), from_numpy(b) if b is not None else None, stride=case[5], padding=case[6]).to_numpy()
        rec.update({f"c{i}_x": x, f"c{i}_w": w, f"c{i}_out": y, f"c{i}_case": np.array(case)})
        if b is not None:
            rec[f"c{i}_b"] = b

    h, q_len, kv_len, d = R.FIXTURE_ATTN
    q, k, v = R.make_attn_case((h, h, q_len, kv_len, d), seed=R.FIXTURE_SEED + 2)
    q4, k4, v4 = (from_numpy(np.ascontiguousarray(a[None])) for a in (q, k, v))
    scores = batched_matmul(q4, k4.transpose(0, 1, 3, 2)) * (1.0 / np.sqrt(d))
    rec.update(a_q=q, a_k=k, a_v=v, a_out=batched_matmul(softmax(scores), v4).to_numpy()[0])

    path = os.path.join(HERE, "g10_whisper.npz")
    np.savez_compressed(path, **rec)
    print({k: v.shape for k, v in rec.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
