"""NumPy restatement of the Whisper decoder (reference: src/pygpukit/asr/whisper/decoder.py; the authority is the reference's own
CPU path, recorded in tests/golden/g11_whisper_decoder.npz by gen_whisper_decoder_golden.py) and of the ln_linear op:

    forward   x = embed_tokens[ids] + embed_positions[:S];  per layer
                  x += out_proj(causal_attention(q, k, v of layer_norm(x)))
                  x += out_proj(attention(q of layer_norm(x); k, v of the encoder states))      every encoder row visible
                  x += fc2(gelu(fc1(layer_norm(x))));   logits = layer_norm(x) @ proj_out^T     tanh GELU, k_proj without bias
    step      the same computation for ONE token against cached K / V rows (self) and K / V projected once (cross): it must
              equal `forward`'s row for the same prefix
    ln_linear out[m, n] = act(LN(x[m]) . w[n] + bias[n]) + residual[m, n]

`dtype` is the type every operand, product and sum is held in: float64 (the oracle) or float32 (the yardstick for what fp32
arithmetic alone costs); `round_dtype` "bf16" / "f16" first rounds weights and encoder states to what the device holds.
`mutate` plants ONE known error, for the test that shows the bars separate right from wrong.  drop_k_bias_zero is the exception
that proves a rule: a bias on k shifts every score of a row alike and softmax does not see it."""

from __future__ import annotations

import numpy as np

from tests.attn_stair_ref import from_words, round_to, to_words  # noqa: F401  (re-exported for the GPU tests)
from tests.whisper_ref import gelu, layernorm

MUTATIONS = ("cross_is_causal", "position_off_by_one", "stale_cache_row", "drop_k_bias_zero", "skip_final_norm", "v_bias_on_q")

FIXTURE_SEED = 156                       # chosen by gen_whisper_decoder_golden.py's conditions (see there)
FIXTURE_ENC_ROWS = 37
FIXTURE_IDS = (201, 7, 150, 33, 92)     # the teacher-forced sequence whose logits are recorded
FIXTURE_STEPS = 20                      # generate(max_length=20)


def fixture_config():
    """The configuration tests/golden/g11_whisper_decoder.npz was recorded with; vocabulary 203 leaves a row tail at every GEMV
    grouping.  No token is EOS within reach: eos_token_id is the last id and the seed's greedy run does not produce it."""
    from pygpukit_amd.asr.whisper import WhisperConfig

    return WhisperConfig(d_model=128, encoder_layers=2, decoder_layers=2, encoder_attention_heads=2, decoder_attention_heads=2,
                         encoder_ffn_dim=256, decoder_ffn_dim=256, vocab_size=203, num_mel_bins=16, max_source_positions=37,
                         max_target_positions=24, bos_token_id=202, eos_token_id=202, pad_token_id=200, decoder_start_token_id=201)


def make_decoder_weights(cfg, seed: int) -> dict:
    """Every decoder tensor under its Hugging Face name, float32, from np.random.default_rng(seed).  k_proj has no bias;
    proj_out.weight is UNTIED and the embeddings have unit scale: with the tied table the start token's own row wins every
    argmax and greedy decoding repeats it forever (tried on the reference's CPU path)."""
    rng = np.random.default_rng(seed)
    d, f, v = cfg.d_model, cfg.decoder_ffn_dim, cfg.vocab_size

    def mat(rows, cols):
        return (rng.standard_normal((rows, cols)) / np.sqrt(cols)).astype(np.float32)

    def vec(n, centre=0.0):
        return (centre + 0.1 * rng.standard_normal(n)).astype(np.float32)

    p = "model.decoder."
    t = {p + "embed_tokens.weight": rng.standard_normal((v, d)).astype(np.float32),
         p + "embed_positions.weight": rng.standard_normal((cfg.max_target_positions, d)).astype(np.float32),
         p + "layer_norm.weight": vec(d, 1.0), p + "layer_norm.bias": vec(d), "proj_out.weight": mat(v, d)}
    for i in range(cfg.decoder_layers):
        q = f"{p}layers.{i}."
        for attn in ("self_attn", "encoder_attn"):
            for name in ("q_proj", "k_proj", "v_proj", "out_proj"):
                t[q + f"{attn}.{name}.weight"] = mat(d, d)
                if name != "k_proj":
                    t[q + f"{attn}.{name}.bias"] = vec(d)
            t[q + f"{attn}_layer_norm.weight"], t[q + f"{attn}_layer_norm.bias"] = vec(d, 1.0), vec(d)
        t[q + "fc1.weight"], t[q + "fc1.bias"] = mat(f, d), vec(f)
        t[q + "fc2.weight"], t[q + "fc2.bias"] = mat(d, f), vec(d)
        t[q + "final_layer_norm.weight"], t[q + "final_layer_norm.bias"] = vec(d, 1.0), vec(d)
    return t


def make_encoder_states(cfg, rows: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).standard_normal((1, rows, cfg.d_model)).astype(np.float32)


def _softmax_rows(s):
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    return p / p.sum(axis=-1, keepdims=True)


class DecoderRef:
    """The decoder on one set of weights: forward(ids, enc) and the cached step()."""

    def __init__(self, cfg, tensors: dict, dtype=np.float64, round_dtype: str = "f32", mutate=None):
        if mutate is not None and mutate not in MUTATIONS:
            raise ValueError(f"unknown mutation {mutate!r}")
        self.cfg, self.dtype, self.round_dtype, self.mutate = cfg, dtype, round_dtype, mutate
        self.w = {k: np.asarray(round_to(v, round_dtype), dtype) for k, v in tensors.items()}
        self.H, self.d = cfg.decoder_attention_heads, cfg.d_model
        self.hd = self.d // self.H
        self.proj_out = self.w.get("proj_out.weight", self.w["model.decoder.embed_tokens.weight"])
        self._cross = None
        self._self = None

    # ---- pieces ----------------------------------------------------------------------------------------------------
    def _lin(self, a, prefix: str, name: str):
        w = self.w[prefix + name + ".weight"]
        b = self.w.get(prefix + name + ".bias")
        if b is None:                                        # k_proj: zeros
            b = np.zeros(w.shape[0], self.dtype)
            if self.mutate == "drop_k_bias_zero":
                b = self.w[prefix + name.replace("k_proj", "v_proj") + ".bias"]
        if self.mutate == "v_bias_on_q" and name.endswith("q_proj"):        # the biases of a fused q | k | v vector in the wrong order
            b = self.w[prefix + name.replace("q_proj", "v_proj") + ".bias"]
        return a @ w.T + b

    def _ln(self, x, prefix: str):
        return layernorm(x, self.w[prefix + ".weight"], self.w[prefix + ".bias"])

    def _heads(self, a):
        return a.reshape(a.shape[0], self.H, self.hd).transpose(1, 0, 2)        # [rows, d] -> [H, rows, hd]

    def _attend(self, q, k, v, causal_offset=None):
        """q [H, Sq, hd] over k / v [H, Sk, hd]; causal_offset: query row i sees keys 0 .. causal_offset + i."""
        s = np.einsum("hqd,hkd->hqk", q, k) * self.dtype(1.0 / np.sqrt(self.hd))
        if causal_offset is not None:
            visible = np.arange(k.shape[1])[None, :] <= causal_offset + np.arange(q.shape[1])[:, None]
            s = np.where(visible[None], s, -np.inf)
        out = np.einsum("hqk,hkd->hqd", _softmax_rows(s), v)
        return out.transpose(1, 0, 2).reshape(q.shape[1], self.d)

    def _embed(self, ids, first_pos: int):
        pos = first_pos + np.arange(len(ids)) + (1 if self.mutate == "position_off_by_one" else 0)
        pos = np.minimum(pos, self.cfg.max_target_positions - 1)
        return self.w["model.decoder.embed_tokens.weight"][np.asarray(ids)] + self.w["model.decoder.embed_positions.weight"][pos]

    def _logits(self, x):
        if self.mutate != "skip_final_norm":
            x = self._ln(x, "model.decoder.layer_norm")
        out = x @ self.proj_out.T
        assert out.dtype == self.dtype
        return out

    # ---- teacher-forced forward ---------------------------------------------------------------------------------------
    def forward(self, ids, enc) -> np.ndarray:
        """ids [S], enc [S_enc, d] -> logits [S, vocab]."""
        enc = np.asarray(round_to(enc, self.round_dtype), self.dtype)
        x = self._embed(ids, 0)
        S = x.shape[0]
        for i in range(self.cfg.decoder_layers):
            p = f"model.decoder.layers.{i}."
            h = self._ln(x, p + "self_attn_layer_norm")
            q, k, v = (self._heads(self._lin(h, p, f"self_attn.{n}_proj")) for n in "qkv")
            x = x + self._lin(self._attend(q, k, v, causal_offset=0), p, "self_attn.out_proj")
            h = self._ln(x, p + "encoder_attn_layer_norm")
            q = self._heads(self._lin(h, p, "encoder_attn.q_proj"))
            k, v = (self._heads(self._lin(enc, p, f"encoder_attn.{n}_proj")) for n in "kv")
            cross_offset = 0 if self.mutate == "cross_is_causal" else None            # encoder row j hidden from query i < j
            x = x + self._lin(self._attend(q, k, v, causal_offset=cross_offset), p, "encoder_attn.out_proj")
            h = self._ln(x, p + "final_layer_norm")
            x = x + self._lin(gelu(self._lin(h, p, "fc1")), p, "fc2")
        return self._logits(x)

    # ---- cached step ----------------------------------------------------------------------------------------------------
    def set_encoder_states(self, enc) -> None:
        enc = np.asarray(round_to(enc, self.round_dtype), self.dtype)
        self._cross = []
        for i in range(self.cfg.decoder_layers):
            p = f"model.decoder.layers.{i}."
            self._cross.append(tuple(self._heads(self._lin(enc, p, f"encoder_attn.{n}_proj")) for n in "kv"))
        T = self.cfg.max_target_positions
        self._self = [(np.zeros((self.H, T, self.hd), self.dtype), np.zeros((self.H, T, self.hd), self.dtype))
                      for _ in range(self.cfg.decoder_layers)]

    def step(self, token: int, position: int) -> np.ndarray:
        """token at `position` against self-cache rows 0 .. position-1 (its own row is written first) -> logits [vocab]."""
        x = self._embed([token], position)
        for i in range(self.cfg.decoder_layers):
            p = f"model.decoder.layers.{i}."
            h = self._ln(x, p + "self_attn_layer_norm")
            q, k, v = (self._heads(self._lin(h, p, f"self_attn.{n}_proj")) for n in "qkv")
            kc, vc = self._self[i]
            row = 0 if self.mutate == "stale_cache_row" else position        # the position is ignored: rows 1.. keep what they held
            kc[:, row], vc[:, row] = k[:, 0], v[:, 0]
            x = x + self._lin(self._attend(q, kc[:, :position + 1], vc[:, :position + 1]), p, "self_attn.out_proj")
            h = self._ln(x, p + "encoder_attn_layer_norm")
            q = self._heads(self._lin(h, p, "encoder_attn.q_proj"))
            ck, cv = self._cross[i]
            n_vis = min(position + 1, ck.shape[1]) if self.mutate == "cross_is_causal" else ck.shape[1]
            x = x + self._lin(self._attend(q, ck[:, :n_vis], cv[:, :n_vis]), p, "encoder_attn.out_proj")
            h = self._ln(x, p + "final_layer_norm")
            x = x + self._lin(gelu(self._lin(h, p, "fc1")), p, "fc2")
        return self._logits(x)[0]

    def generate(self, enc, max_length: int, prompt_ids=None, use_cache: bool = True, return_logits: bool = False):
        """Greedy: the reference's loop (start token or prompt, argmax, stop after EOS)."""
        cfg = self.cfg
        tokens = [int(t) for t in prompt_ids] if prompt_ids is not None else [cfg.decoder_start_token_id]
        max_length = min(max_length, cfg.max_target_positions)
        rows = []
        if use_cache:
            self.set_encoder_states(enc)
            logits = None
            for pos, t in enumerate(tokens):
                logits = self.step(t, pos)
        while len(tokens) < max_length:
            if not use_cache:
                logits = self.forward(tokens, enc)[-1]
            rows.append(logits)
            nxt = int(np.argmax(logits))
            tokens.append(nxt)
            if nxt == cfg.eos_token_id or len(tokens) >= max_length:
                break
            if use_cache:
                logits = self.step(nxt, len(tokens) - 1)
        return (tokens, np.array(rows)) if return_logits else tokens


def top2_gap(logits) -> float:
    s = np.sort(np.asarray(logits, np.float64))
    return float(s[-1] - s[-2])


# ---- ln_linear ---------------------------------------------------------------------------------------------------------------
# (M, K, N) of tests/test_ln_linear_gpu.py with what each reaches; the kernels stream 4 rows per wave, 16 per workgroup, and a
# lane's first 16-byte chunk covers k < 512 (16-bit) / 256 (float32)
LN_SHAPES = ((1, 128, 203),      # fixture shape: a tail at every row grouping
             (1, 64, 1),         # one output; K below one chunk per wave
             (3, 200, 37),       # 25 chunks: lanes 25.. of the wave hold none
             (3, 204, 37),       # K % 8 != 0: generic path
             (8, 128, 384),      # eight rows
             (1, 1280, 70),      # Whisper-large d_model: three chunks per lane
             (2, 5120, 40),      # Whisper-large FFN width
             (8, 5120, 16),      # fp32 image 160 KB, dtype image 80 KB (16-bit): generic kernel at eight rows
             (4, 5120, 24),      # no norm, 16-bit: fp32 image 80 KB > 64 KB, rows held in the dtype (40 KB); with a norm: generic
             (8, 2048, 24),      # fp32 image exactly 64 KB: fits, but with a norm gamma / beta no longer fit beside it
             (1, 8, 5),          # one 16-byte chunk in all
             (1, 512, 24), (1, 520, 24), (1, 256, 24), (1, 264, 24))    # the chunk boundary of the peeled first trip, both widths
LN_VARIANTS = ("plain", "bias", "ln", "ln_bias_gelu", "bias_residual", "residual_alias_out", "ln_bias_residual")


def ln_case_seed(shape, variant: str) -> int:
    return 4000 + 7 * sum((i + 1) * 131 * int(v) for i, v in enumerate(shape)) + LN_VARIANTS.index(variant)


def make_ln_case(shape, variant: str, round_dtype: str = "f32") -> dict:
    """Operands of one case as float32 arrays already rounded to `round_dtype` (the values the device holds).  LN cases draw
    x ~ N(0.3, 1), so that x - mean does not cancel."""
    m, k, n = shape
    rng = np.random.default_rng(ln_case_seed(shape, variant))
    norm = variant.startswith("ln")
    c = {"x": (0.3 if norm else 0.0) + rng.standard_normal((m, k)), "w": rng.standard_normal((n, k)) / np.sqrt(k)}
    c["bias"] = 0.5 * rng.standard_normal(n) if "bias" in variant else None
    c["gamma"] = 1.0 + 0.1 * rng.standard_normal(k) if norm else None
    c["beta"] = 0.1 * rng.standard_normal(k) if norm else None
    c["residual"] = rng.standard_normal((m, n)) if "residual" in variant else None
    c["activation"] = "gelu" if "gelu" in variant else None
    return {key: (round_to(np.asarray(v, np.float32), round_dtype) if isinstance(v, np.ndarray) else v) for key, v in c.items()}


def ln_linear(c: dict, dtype=np.float64, eps: float = 1e-5, parts: bool = False):
    """The op on a case of make_ln_case.  parts=True also returns what the bar is built from: the pre-activation value and
    sum |x^ w| + |b| (the scale of the accumulation error)."""
    cast = lambda a: None if a is None else np.asarray(a, dtype)        # noqa: E731
    x, w, bias, gamma, beta, res = (cast(c[k]) for k in ("x", "w", "bias", "gamma", "beta", "residual"))
    xh = layernorm(x, gamma, beta, eps) if gamma is not None else x
    pre = xh @ w.T
    if bias is not None:
        pre = pre + bias
    out = gelu(pre) if c["activation"] == "gelu" else pre
    if res is not None:
        out = out + res
    assert out.dtype == dtype
    if not parts:
        return out
    scale = np.abs(xh) @ np.abs(w).T + (np.abs(bias) if bias is not None else 0.0)
    return out, pre, scale


def ln_bar(c: dict, round_dtype: str, n_ln_factor: float = 1.0) -> np.ndarray:
    """Elementwise bar of tests/test_ln_linear_gpu.py, from the float64 oracle:
        accumulation  (n + n_ln) 2^-24 (sum |x^ w| + |b| + |r|), n = K + 2 (doubled in float32: the products round too),
                      n_ln = 0 without the norm, 2K + 8 with it (two K-term fp32 sums and the normalisation's roundings move
                      each x^ by at most that many ulps)
        GELU          the pre-activation bar x 1.13 (max |gelu'|) + 2^-21 |ref| for the device tanhf
        output        2^-8 |ref| (bf16), 2^-11 |ref| (f16), nothing for float32."""
    ref, pre, scale = ln_linear(c, parts=True)
    k = c["x"].shape[1]
    n = (k + 2) * (2 if round_dtype == "f32" else 1)
    n_ln = n_ln_factor * (2 * k + 8) if c["gamma"] is not None else 0
    bar = (n + n_ln) * 2.0 ** -24 * scale
    if c["activation"] == "gelu":
        bar = 1.13 * bar + 2.0 ** -21 * np.abs(ref)
    if c["residual"] is not None:
        bar = bar + (n + n_ln) * 2.0 ** -24 * np.abs(np.asarray(c["residual"], np.float64))
    return bar + {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}[round_dtype] * np.abs(ref)
