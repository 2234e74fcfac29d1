"""Records tests/golden/g16_text_encoders.npz: the text encoders' outputs from the reference package's own CPU path and from
HuggingFace transformers in float64.

    python tests/golden/gen_text_encoder_golden.py <path to the reference's src directory>

Only this generator imports the reference (`pygpukit`) and `transformers`; the tests read the fixture.  The fixture stores seeds,
inputs and outputs; the weights are regenerated from tests/t5_ref.py and tests/clip_ref.py make_weights(fixture_config(), seed).
HF models are built from a config object only (HF_HUB_OFFLINE=1, no from_pretrained) and loaded through load_state_dict.

Recorded:
  * bucket_deltas (-600..600), buckets_ref: the reference's T5Encoder._relative_position_bucket; buckets_hf:
    T5Attention._relative_position_bucket.  The generator asserts that they are equal, and equal on a 512 x 512 position grid;
  * t5_ids, t5_mask; t5_ref_out: the reference's T5Encoder.forward (float32: attention scale 1/sqrt(d_kv), ReLU gate, -1e9 mask);
    t5_hf_out: T5EncoderModel (v1.1, gated-gelu) in float64, same weights, same mask;
  * clip_ids, clip_mask; clip_pooled: CLIPTextModel in float64 with the padding mask; clip_hidden, clip_pooled_nomask: without it.
    The generator asserts that the two pooled outputs, and every hidden row up to the EOS, are equal (under the causal mask a row
    cannot see the padding after it).
transformers computes T5's softmax in float32 whatever the model's dtype, so t5_hf_out is float64 arithmetic around a float32
softmax: the float64 restatement is about 1e-7 from it, not 1e-16."""

from __future__ import annotations

import os
import sys

os.environ["HF_HUB_OFFLINE"] = "1"

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
from tests import clip_ref as C  # noqa: E402
from tests import t5_ref as T  # noqa: E402

T5_SEED, CLIP_SEED = 1601, 1602


def _load(model, weights: dict, torch, strip: str = "") -> None:
    have = model.state_dict()
    sd = {}
    for name in have:
        src = name if name in weights else strip + name
        if src not in weights and name.startswith(strip):
            src = name[len(strip):]
        sd[name] = torch.tensor(np.asarray(weights[src], np.float64))
    model.load_state_dict(sd, strict=True)


def main(ref_src: str) -> None:
    sys.path.insert(0, ref_src)
    import torch
    from pygpukit.core.factory import from_numpy
    from pygpukit.diffusion.text_encoders.t5 import T5Encoder
    from transformers import CLIPTextConfig, CLIPTextModel, T5Config, T5EncoderModel
    from transformers.models.t5.modeling_t5 import T5Attention

    out = {"t5_seed": np.int64(T5_SEED), "clip_seed": np.int64(CLIP_SEED)}

    # ---- buckets ----
    deltas = np.arange(-600, 601)
    ref_enc = T5Encoder(hidden_size=8, num_layers=0, num_heads=1, d_ff=8)
    b_ref = np.asarray(ref_enc._relative_position_bucket(deltas, bidirectional=True, num_buckets=32, max_distance=128))
    b_hf = T5Attention._relative_position_bucket(torch.tensor(deltas), bidirectional=True, num_buckets=32, max_distance=128).numpy()
    assert np.array_equal(b_ref, b_hf), "reference and HF buckets differ"
    grid = np.arange(512)[None, :] - np.arange(512)[:, None]
    assert np.array_equal(np.asarray(ref_enc._relative_position_bucket(grid)),
                          T5Attention._relative_position_bucket(torch.tensor(grid), True, 32, 128).numpy())
    out.update(bucket_deltas=deltas.astype(np.int32), buckets_ref=b_ref.astype(np.int32), buckets_hf=b_hf.astype(np.int32))

    # ---- T5 ----
    cfg = T.fixture_config()
    w = T.make_weights(cfg, T5_SEED)
    ids, mask = T.make_inputs(cfg, T5_SEED)
    enc = T5Encoder(hidden_size=cfg["d_model"], num_layers=cfg["num_layers"], num_heads=cfg["num_heads"], d_ff=cfg["d_ff"],
                    max_length=cfg["seq"], weights={n: from_numpy(a) for n, a in w.items()})
    t5_ref_out = enc.forward(from_numpy(ids), from_numpy(mask)).to_numpy()
    hf_cfg = T5Config(vocab_size=cfg["vocab_size"], d_model=cfg["d_model"], d_kv=cfg["d_kv"], d_ff=cfg["d_ff"], num_layers=cfg["num_layers"],
                      num_heads=cfg["num_heads"], relative_attention_num_buckets=cfg["num_buckets"],
                      relative_attention_max_distance=cfg["max_distance"], dropout_rate=0.0, layer_norm_epsilon=cfg["eps"],
                      feed_forward_proj="gated-gelu", is_encoder_decoder=False, use_cache=False, tie_word_embeddings=False)
    model = T5EncoderModel(hf_cfg).double().eval()
    _load(model, w, torch)
    with torch.no_grad():
        t5_hf_out = model(input_ids=torch.tensor(ids), attention_mask=torch.tensor(mask)).last_hidden_state.numpy()
    out.update(t5_ids=ids.astype(np.int32), t5_mask=mask.astype(np.int8), t5_ref_out=t5_ref_out.astype(np.float32),
               t5_hf_out=t5_hf_out.astype(np.float32))

    # ---- CLIP ----
    ccfg = C.fixture_config()
    cw = C.make_weights(ccfg, CLIP_SEED)
    cids, cmask = C.make_inputs(ccfg, CLIP_SEED)
    hf_ccfg = CLIPTextConfig(vocab_size=ccfg["vocab_size"], hidden_size=ccfg["hidden_size"], intermediate_size=ccfg["intermediate_size"],
                             num_hidden_layers=ccfg["num_layers"], num_attention_heads=ccfg["num_heads"],
                             max_position_embeddings=ccfg["max_positions"], hidden_act=ccfg["hidden_act"], layer_norm_eps=ccfg["eps"],
                             attention_dropout=0.0, pad_token_id=ccfg["pad_token_id"], bos_token_id=ccfg["bos_token_id"],
                             eos_token_id=ccfg["eos_token_id"])
    cmodel = CLIPTextModel(hf_ccfg).double().eval()
    _load(cmodel, cw, torch, strip=C.PREFIX)
    with torch.no_grad():
        r_mask = cmodel(input_ids=torch.tensor(cids), attention_mask=torch.tensor(cmask))
        r_nomask = cmodel(input_ids=torch.tensor(cids))
    pooled, pooled_nomask = r_mask.pooler_output.numpy(), r_nomask.pooler_output.numpy()
    assert np.array_equal(pooled, pooled_nomask), "the padding mask changed the pooled output"
    # rows up to the EOS cannot see the padding either; the rows after it can, so clip_hidden is the run WITHOUT the mask (the classes
    # here ignore it, as the reference's class does)
    hid, hid_mask = r_nomask.last_hidden_state.numpy(), r_mask.last_hidden_state.numpy()
    for b_, e in enumerate(ccfg["eos_at"]):
        assert np.array_equal(hid[b_, :e + 1], hid_mask[b_, :e + 1]), "the padding mask changed a row before the EOS"
    out.update(clip_ids=cids.astype(np.int32), clip_mask=cmask.astype(np.int8), clip_hidden=hid.astype(np.float32),
               clip_pooled=pooled.astype(np.float32), clip_pooled_nomask=pooled_nomask.astype(np.float32))

    path = os.path.join(HERE, "g16_text_encoders.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")
    for n, a in out.items():
        print(f"  {n}: {np.asarray(a).shape} {np.asarray(a).dtype}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
