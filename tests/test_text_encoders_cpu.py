"""Host-side tests of the relative-position bias and the text encoders: the NumPy restatements (tests/t5_ref.py, tests/clip_ref.py)
against the recorded fixture, the bucket function against the reference's recorded buckets, the clamp-radius claim behind the bias
table, the C ABI of the new op, the plan decisions, the tokenizer fallbacks, the mask and pooled-position rules, and FluxPipeline's
behaviour with and without encoders.  No GPU: nothing here launches a kernel."""

from __future__ import annotations

import os
import re

import numpy as np
import pytest

from tests import clip_ref as C
from tests import t5_ref as T
from tests.conftest import ROOT, load_golden, rel_err

g16 = load_golden("g16_text_encoders.npz")


# ---- restatements against the fixture ----------------------------------------------------------------------------------------

def test_t5_restatement_equals_the_fixture_in_both_modes():
    cfg = T.fixture_config()
    w = T.make_weights(cfg, int(g16["t5_seed"]))
    ids, mask = g16["t5_ids"].astype(np.int64), g16["t5_mask"].astype(np.int64)
    assert np.array_equal(T.make_inputs(cfg, int(g16["t5_seed"]))[0], ids) and mask.sum(axis=1).tolist() == list(cfg["valid"])
    # HF computes T5's softmax in float32 whatever the model's dtype, and the fixture is stored as float32: 1e-7, not 1e-16.
    # The reference's whole path is float32: its distance is the float32 restatement's own.
    e_hf = rel_err(T.t5_forward(cfg, w, ids, mask, "hf"), g16["t5_hf_out"])
    ref64 = T.t5_forward(cfg, w, ids, mask, "reference")
    e_ref = rel_err(ref64, g16["t5_ref_out"])
    yard = rel_err(T.t5_forward(cfg, w, ids, mask, "reference", dtype=np.float32), ref64)
    print(f"T5 restatement vs fixture: hf {e_hf:.3e}, reference {e_ref:.3e} (float32 restatement vs float64: {yard:.3e})")
    assert e_hf <= 5e-7 and e_ref <= 4 * yard <= 1e-5
    assert rel_err(T.t5_forward(cfg, w, ids, mask, "reference"), g16["t5_hf_out"]) > 0.05       # the modes differ
    assert rel_err(T.t5_forward(cfg, w, ids, None, "hf")[1], g16["t5_hf_out"][1]) > 0.05         # the mask matters


def test_clip_restatement_equals_the_fixture():
    cfg = C.fixture_config()
    w = C.make_weights(cfg, int(g16["clip_seed"]))
    ids = g16["clip_ids"].astype(np.int64)
    assert np.array_equal(C.make_inputs(cfg, int(g16["clip_seed"]))[0], ids)
    hidden, pooled = C.clip_forward(cfg, w, ids)
    e_h, e_p = rel_err(hidden, g16["clip_hidden"]), rel_err(pooled, g16["clip_pooled"])
    print(f"CLIP restatement vs fixture: hidden {e_h:.3e}, pooled {e_p:.3e}")
    assert e_h <= 1e-7 and e_p <= 1e-7                                   # float64 against float64 stored as float32
    assert np.array_equal(g16["clip_pooled"], g16["clip_pooled_nomask"])


# ---- the bias ------------------------------------------------------------------------------------------------------------------

def test_relpos_bucket_equals_the_recorded_reference_buckets():
    from pygpukit_amd.ops.nn.relpos import relpos_bucket

    deltas = g16["bucket_deltas"].astype(np.int64)
    assert deltas[0] == -600 and deltas[-1] == 600
    assert np.array_equal(g16["buckets_ref"], g16["buckets_hf"])
    assert np.array_equal(relpos_bucket(deltas), g16["buckets_ref"])
    assert np.array_equal(T.relpos_bucket(deltas), g16["buckets_ref"])
    grid = deltas[None, :300] - deltas[:200, None]
    assert np.array_equal(relpos_bucket(grid), T.relpos_bucket(grid))
    # saturation: what makes a table of 2R + 1 entries enough.  Keys at or beyond +128 (after the query) share bucket 31, keys at or
    # beyond -128 bucket 15, in the reference's function and in HF's alike.
    b = g16["buckets_ref"]
    assert (b[deltas >= 128] == 31).all() and (b[deltas <= -128] == 15).all()


@pytest.mark.parametrize("q_len,kv_len", [(1, 1), (1, 130), (130, 97), (512, 300), (300, 512), (512, 512)])
def test_bias_table_expands_to_the_dense_bias(q_len, kv_len):
    """The clamp-radius claim: table[h, clamp(j - i, -R, R) + R] IS weight[bucket(j - i), h] at every sequence length."""
    from pygpukit_amd.ops.nn.relpos import relpos_bias_table_host, relpos_compute_bias_host

    weight = np.random.default_rng(q_len + kv_len).standard_normal((32, 5)).astype(np.float32)
    table = relpos_bias_table_host(weight, True, 128)
    assert table.shape == (5, 257) and table.dtype == np.float32 and table.flags.c_contiguous
    dense = T.dense_bias(weight, q_len, kv_len)
    assert np.array_equal(relpos_compute_bias_host(table, q_len, kv_len), dense)
    assert np.array_equal(T.expand_table(T.bias_table(weight), q_len, kv_len), dense)
    assert np.array_equal(table, T.bias_table(weight))
    # delta is key - query: a key to the RIGHT of the query (j > i) reads the upper half of the table
    if kv_len > 1:
        assert dense[0, 0, 1] == weight[T.relpos_bucket(1), 0] == table[0, 129]


def test_relbias_c_abi_is_declared_and_bound():
    from pygpukit_amd import _hip

    header = open(os.path.join(ROOT, "include", "pgk_hip.h")).read()
    for name, table in (("pgk_sdpa_relbias", _hip._PROTOS), ("pgk_relbias_plan", {n: a for n, (a, _) in _hip._NON_STATUS.items()})):
        m = re.search(r"\b" + name + r"\(([^;]*?)\);", header, re.S)
        assert m, f"{name} is not declared in include/pgk_hip.h"
        assert len(m.group(1).split(",")) == len(table[name]), name
        assert name in _hip.EXPORTED_SYMBOLS
    # the six strides follow scale, as in pgk_sdpa_noncausal
    assert _hip._PROTOS["pgk_sdpa_relbias"][12:18] == _hip._PROTOS["pgk_sdpa_noncausal"][10:16] == [_hip._I64] * 6
    makefile = open(os.path.join(ROOT, "pygpukit_amd", "csrc", "Makefile")).read()
    assert "ops_relbias.hip" in makefile
    import pygpukit_amd
    from pygpukit_amd import ops

    for n in ("relpos_bucket", "relpos_bias_table", "relpos_compute_bias", "sdpa_relbias", "sdpa_relbias_strided", "relbias_plan"):
        assert getattr(pygpukit_amd, n) is getattr(ops, n) is getattr(ops.nn, n)


def test_relbias_plan_host_decisions():
    from pygpukit_amd.diffusion import t5_plan
    from pygpukit_amd.ops.nn import relbias_plan

    for dt in ("bfloat16", "float16"):
        for d in (64, 128):
            assert relbias_plan(d, 128, dt) == "relbias_flash"
            assert relbias_plan(d, 0, dt) == relbias_plan(d, 1024, dt) == "relbias_flash"
            assert relbias_plan(d, 1025, dt) == "relbias_rows"
            assert relbias_plan(d, 128, dt, aligned=False) == "relbias_rows"
        for d in (32, 80, 96, 256):
            assert relbias_plan(d, 128, dt) == "relbias_rows"
    for d in (64, 128, 80):
        assert relbias_plan(d, 128, "float32") == "relbias_rows"
    for bad in ((0, 128), (257, 128), (64, -1)):
        with pytest.raises(ValueError, match="pgk_relbias_plan"):
            relbias_plan(*bad, "bfloat16")
    xxl = t5_plan(4096, 64, 64, 10240, 512, "bfloat16")
    assert xxl == {"launches_per_layer": 10, "attention": "relbias_flash", "table_bytes": 64 * 257 * 4, "dense_bias_bytes": 64 * 512 * 512 * 4}
    assert t5_plan(4096, 64, 64, 10240, 512, "float32", "relu")["launches_per_layer"] == 12


# ---- text ------------------------------------------------------------------------------------------------------------------

def test_tokenizer_fallbacks_are_the_reference_rules():
    from pygpukit_amd.diffusion import CLIPTextEncoder, T5Encoder, T5XXLEncoder

    t5 = T5XXLEncoder()
    assert (t5.hidden_size, t5.num_layers, t5.num_heads, t5.d_ff, t5.max_length) == (4096, 24, 64, 10240, 512)
    ids, mask = t5.tokenize("a cat")
    want = [ord(c) % 32000 for c in "a cat"] + [1]
    assert ids.shape == mask.shape == (1, 512) and ids.dtype == mask.dtype == np.int64
    assert ids[0, :6].tolist() == want and not ids[0, 6:].any() and mask[0].tolist() == [1] * 6 + [0] * 506
    ids, mask = T5Encoder(max_length=4).tokenize(["abcdefgh", "猫"])
    assert ids.tolist() == [[97, 98, 99, 1], [ord("猫") % 32000, 1, 0, 0]] and mask.tolist() == [[1, 1, 1, 1], [1, 1, 0, 0]]
    clip = CLIPTextEncoder()
    ids, mask = clip.tokenize("a cat")
    assert ids.shape == (1, 77) and ids[0, :7].tolist() == [49406, 97, 32, 99, 97, 116, 49407] and mask[0].sum() == 7
    ids, _ = clip.tokenize("x" * 100)
    assert ids[0, 0] == 49406 and ids[0, 76] == 49407 and (ids[0, 1:76] == ord("x")).all()
    with pytest.raises(RuntimeError, match="no weights"):
        t5.forward(ids)


def test_tokenizer_json_goes_through_the_tokenizers_library(tmp_path):
    tokenizers = pytest.importorskip("tokenizers")
    from pygpukit_amd.diffusion import T5Encoder

    vocab = {"[UNK]": 0, "a": 5, "cat": 9}
    tok = tokenizers.Tokenizer(tokenizers.models.WordLevel(vocab, unk_token="[UNK]"))
    tok.pre_tokenizer = tokenizers.pre_tokenizers.Whitespace()
    path = tmp_path / "tokenizer.json"
    tok.save(str(path))
    for given in (tok, str(path), str(tmp_path)):
        ids, mask = T5Encoder(max_length=4, tokenizer=given).tokenize("a cat dog")
        assert ids.tolist() == [[5, 9, 0, 0]] and mask.tolist() == [[1, 1, 1, 0]]


def test_prefix_mask_rule():
    from pygpukit_amd.diffusion.text_encoders.t5 import prefix_lengths

    assert prefix_lengths(None, 2, 5) == [5, 5]
    assert prefix_lengths(np.array([[1, 1, 1, 0, 0], [1, 1, 1, 1, 1]], np.int8), 2, 5) == [3, 5]
    for bad in ([[1, 0, 1, 0, 0], [1, 1, 1, 1, 1]], [[0, 0, 0, 0, 0], [1, 1, 1, 1, 1]], [[0, 1, 1, 1, 1], [1, 1, 1, 1, 1]]):
        with pytest.raises(ValueError, match="prefix mask"):
            prefix_lengths(np.array(bad), 2, 5)
    with pytest.raises(ValueError):
        prefix_lengths(np.ones((2, 4)), 2, 5)
    with pytest.raises(ValueError):
        prefix_lengths(np.full((2, 5), 2), 2, 5)


def test_pooled_position_rule():
    from pygpukit_amd.diffusion.text_encoders.clip import pooled_position

    ids = np.array([49406, 320, 49407, 49407, 0, 0])
    assert pooled_position(ids, 49407) == 2 == C.pooled_position(ids, 49407)          # the FIRST eos, not the last row
    assert pooled_position(np.array([1, 7, 9, 3, 9, 0]), 2) == 2                      # eos_token_id == 2: argmax of the ids
    assert pooled_position(np.array([49406, 5, 6]), 49407) == 0                       # no eos: argmax of all-False
    cfg = C.fixture_config()
    for row, at in zip(g16["clip_ids"], cfg["eos_at"]):
        assert pooled_position(row, cfg["eos_token_id"]) == at


# ---- FluxPipeline --------------------------------------------------------------------------------------------------------------

class _Stub:
    def __init__(self, name, log, out):
        self.name, self.log, self.out = name, log, out

    def tokenize(self, text, max_length=None):
        self.log.append((self.name, "tokenize", text, max_length))
        return "ids_" + self.name, "mask_" + self.name

    def forward(self, ids, mask=None):
        self.log.append((self.name, "forward", ids, mask))
        return self.out


class _Transformer:
    class config:
        in_channels = 8


def test_flux_pipeline_with_and_without_encoders():
    from pygpukit_amd.diffusion import FluxPipeline

    bare = FluxPipeline(_Transformer(), None)
    assert bare.text_encoder is None and bare.text_encoder_2 is None
    for call in (lambda: bare.encode_prompt("a cat"), lambda: bare("a cat"), lambda: bare(prompt="a cat"),
                 lambda: FluxPipeline(_Transformer(), None, text_encoder=object())("a cat"), lambda: FluxPipeline.from_pretrained("x")):
        with pytest.raises(NotImplementedError, match="prompt_embeds"):
            call()
    with pytest.raises(NotImplementedError, match="prompt_embeds"):
        FluxPipeline.__new__(FluxPipeline).encode_prompt("a cat")
    log = []
    pipe = FluxPipeline(_Transformer(), None, text_encoder=_Stub("clip", log, ("hidden", "POOLED")), text_encoder_2=_Stub("t5", log, "EMBEDS"))
    assert pipe.encode_prompt("a cat") == ("POOLED", "EMBEDS")
    assert log == [("clip", "tokenize", "a cat", 77), ("clip", "forward", "ids_clip", "mask_clip"), ("t5", "tokenize", "a cat", 512),
                   ("t5", "forward", "ids_t5", "mask_t5")]
    del log[:]
    assert pipe.encode_prompt(["a", "b"], 64, mask_padding=False) == ("POOLED", "EMBEDS")
    assert log[2:] == [("t5", "tokenize", ["a", "b"], 64), ("t5", "forward", "ids_t5", None)]
