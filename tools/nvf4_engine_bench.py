"""bf16, fp8 (w8a16) and NVF4 (w4a16) engines side by side, random-init weights, one process.
usage: nvf4_engine_bench.py [--llama-layers L] [--profile]
  decode   per-step time from graph replay (capture once, replay 64 steps, median of 5 windows) at batch 1, 8 and 64
           on the Qwen3-0.6B shape (28 layers; NVF4 batch 64 = 8 GEMV chunks, each re-reading the weights) and on the
           Llama-3-8B shape with L layers (default 8).  Bytes per step = the algorithmic weight bytes of one
           step (layer linears in their format + the bf16 lm_head); TB/s = bytes / step time.  The Llama shape runs batch
           1 and 4: batch 8 needs 8 activation rows of K = 14336 in LDS (224 KiB), which no format's GEMV chunk has.
  prefill  one 2048-token prompt on Qwen3-0.6B, median of 5 calls after 2 warm-ups.
  --profile: only the NVF4 Llama-shape batch-1 replay (for a kernel-trace run)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pygpukit_amd.llm import synthetic as S  # noqa: E402
from pygpukit_amd.llm.engine import Engine  # noqa: E402
from pygpukit_amd.ops.matmul.nvf4 import quantize_nvf4_nk  # noqa: E402

LIN = ("w_qkv", "w_o", "w_gate_up", "w_down")


def nvf4_layers(bf16_layers):
    out = []
    for lw in bf16_layers:
        d = {k: v for k, v in lw.items() if k not in LIN}
        for name in LIN:
            d[name], d["s" + name[1:]] = quantize_nvf4_nk(lw[name])
        out.append(d)
    return out


def step_bytes(cfg, fmt):
    H, D, I, V = cfg["hidden_size"], cfg["head_dim"], cfg["intermediate_size"], cfg["vocab_size"]
    per_layer = ((cfg["num_heads"] + 2 * cfg["num_kv_heads"]) * D * H + H * cfg["num_heads"] * D + 3 * I * H)
    w = per_layer * cfg["num_layers"]
    lin = {"bf16": 2.0 * w, "fp8": 1.0 * w + 2.0 * w / (128 * 128), "nvf4": w / 2 + w / 32}[fmt]
    return lin + 2.0 * V * H


def replay_ms(eng, B, prompt_len=128, n=64):
    rng = np.random.default_rng(0)
    for b in range(B):
        eng.prefill(rng.integers(0, eng.config["vocab_size"], prompt_len).tolist(), seq=b, want_last_logits=False)
    eng.set_state([1] * B, [prompt_len] * B)
    eng.capture(B)
    eng.replay(8)
    eng.synchronize()
    ts = []
    for _ in range(5):
        eng.set_state([1] * B, [prompt_len] * B)
        eng.reset_log()
        eng.synchronize()
        t0 = time.perf_counter()
        eng.replay(n)
        eng.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3 / n)
    return float(np.median(ts))


def prefill_ms(eng, n=2048):
    prompt = np.random.default_rng(1).integers(0, eng.config["vocab_size"], n).tolist()
    for _ in range(2):
        eng.prefill(prompt)
    ts = []
    for _ in range(5):
        eng.synchronize()
        t0 = time.perf_counter()
        eng.prefill(prompt)
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def engines(cfg, w, max_seq_len, max_batch, fmts=("bf16", "fp8", "nvf4")):
    layers = {"bf16": w["bf16"], "fp8": w["fp8"]}
    if "nvf4" in fmts:
        layers["nvf4"] = nvf4_layers(w["bf16"])
    for f in fmts:
        yield f, Engine(cfg, w["embed"], layers[f], w["final_norm"], None, max_seq_len=max_seq_len, max_batch=max_batch,
                        weight_format=f, use_qk_norm=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--llama-layers", type=int, default=8)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    llama = dict(S.LLAMA3_8B, num_layers=args.llama_layers)
    if args.profile:
        w = S.random_engine_weights(llama, seed=0, fp8=False)
        w["fp8"] = None
        for _, eng in engines(llama, w, 256, 1, fmts=("nvf4",)):
            print(f"profile: llama-{args.llama_layers}L nvf4 b1 {replay_ms(eng, 1):.3f} ms/step", flush=True)
        return
    res = {}
    for name, cfg, batches in (("qwen3-0.6b", S.QWEN3_0_6B, (1, 8, 64)), (f"llama3-8b-{args.llama_layers}L", llama, (1, 4))):
        w = S.random_engine_weights(cfg, seed=0, fp8=True)
        for fmt, eng in engines(cfg, w, 2048 + 64, max(batches)):
            for B in batches:
                ms = replay_ms(eng, B)
                res[(name, fmt, B)] = ms
                by = step_bytes(cfg, fmt)
                print(f"decode {name:16s} {fmt:5s} batch {B:2d}: {ms:7.3f} ms/step  {by / 1e9:6.2f} GB/step  {by / ms / 1e9:5.2f} TB/s",
                      flush=True)
            if name == "qwen3-0.6b":
                ms = prefill_ms(eng)
                res[(name, fmt, "prefill")] = ms
                print(f"prefill {name} {fmt:5s} S=2048: {ms:8.2f} ms", flush=True)
            del eng
        del w
    ln = f"llama3-8b-{args.llama_layers}L"
    r1 = res[(ln, "nvf4", 1)] / res[(ln, "bf16", 1)]
    r2 = res[("qwen3-0.6b", "nvf4", "prefill")] / res[("qwen3-0.6b", "bf16", "prefill")]
    print(f"goal decode: {ln} batch 1 nvf4 / bf16 = {r1:.3f} (goal <= 0.5): {'met' if r1 <= 0.5 else 'missed'}")
    print(f"goal prefill: qwen3-0.6b S=2048 nvf4 / bf16 = {r2:.3f} (goal <= 1.15): {'met' if r2 <= 1.15 else 'missed'}")
    print(f"batch 64 cost: qwen3-0.6b nvf4 {res[('qwen3-0.6b', 'nvf4', 64)]:.3f} ms/step vs bf16 {res[('qwen3-0.6b', 'bf16', 64)]:.3f}"
          f" and nvf4 batch 8 {res[('qwen3-0.6b', 'nvf4', 8)]:.3f}")


if __name__ == "__main__":
    main()
