#!/usr/bin/env python3
"""Headline benchmark: BASELINE.json metric "decode tokens/sec/GPU + prefill TFLOPS, Qwen3-0.6B bf16".

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    (N > 1: one process per GPU with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in the environment - what
    `python -m torch.distributed.run --nproc-per-node N bench.py ...` sets, or any other launcher; nothing here imports torch)

A plain run does what the headline needs and nothing else: weights and engine set up, the prompt prefilled, W + K replayed
steps, the outputs dumped if asked for, one JSON line.  `--full` adds every other measurement described below (config 4,
the extras, the per-kernel roofline, both prefill timings, the CPU baseline) AFTER the headline and the dump, so `value`,
`ms_per_step` and the dumped arrays come out of the same code, in the same order, in both kinds of run.

Headline (`value`) at every N = BASELINE config 2 per GPU: random-init Qwen3-0.6B-shape bf16 weights, a 128-token
prompt prefilled through the MFMA path, then K single-token greedy decode steps, each ONE replay of the whole-step
hipGraph (28 layers incl. KV write + attention -> lm_head -> argmax -> next embedding; token / position in device
memory).  A "step" = one decode token for every sequence resident on the GPU.  For N > 1 every rank holds a replica
(weights broadcast once from rank 0 over RCCL - mandatory: no RCCL, no number, exit code 3) and decodes its own
independent sequence: "weak" scaling, no collective inside the timed region; the token logs are all-gathered over
RCCL after it.  `value` = sequences x K / max-over-ranks wall time, inputs resident in HBM.

With `--full`, BASELINE config 4 (batch 64 decode, data-parallel over the node) runs at EVERY N under `extras.config4`:
  weak    b_local = 8 sequences per GPU (global 8 N),
  strong  b_local = 64 / N sequences per GPU (global 64; N = 1: all 64 on one GPU, one pass over the weights per step),
each with its own barrier + device-sync bracket and max-over-ranks time; values are whole-job tokens/s.

Objects on the JSON line (`full` says which kind of run wrote it; all but `step_roofline` need `--full`):
  roofline         the decode-step kernel with the largest share of the step's device time: algorithmic bytes per
                   launch / its average dispatch duration (start/stop events on every launch of eager steps on the
                   launch stream: the begin -> end interval rocprofv3 --kernel-trace reports), vs 8 TB/s HBM;
                   `traffic` = HBM bytes per launch, only when THIS run is itself a rocprofv3 --pmc pass whose counters a
                   later reduction fills in (null otherwise; the round's measured values are in profiles/README.md).
  roofline_kernels the same row for every kernel of the step (per-launch us, bytes, frac, share of the step).
  step_roofline    whole decode step: algorithmic bytes per token / measured step time.
  prefill          ms, TFLOP/s and fraction of the 2.5 PFLOP/s dense bf16 MFMA peak for the 128-token prompt.
  cpu_baseline     the NumPy oracle (reference-semantics CPU path) timed on this box's host cores, rank 0, N = 1.

--dump-outputs DIR (rank 0) writes, after the timed steps, what the headline path handed back in its last step:
  DIR/logits.npy   float32 [batch, vocab] logits of the last timed decode step (all rows while they fit in 48 MB, otherwise
                   a fixed, seeded sample of rows, listed in DIR/logits_rows.npy),
  DIR/tokens.npy   float64 [warmup + steps, batch] the greedy token log of the replayed steps (the first 4096).
The inputs (weights, prompts) depend only on the arguments, so two builds run with the same arguments compare output for output.
(`--dump-outputs bench_out` is ignored by git.)
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s spec (6.3 TB/s measured copy)
MFMA_BF16_PEAK_TFLOPS = 2500.0  # dense bf16


def algorithmic_bytes_per_token(cfg: dict, ctx: int, weight_format: str) -> dict:
    """weights read once per step + un-expanded bf16 KV rows + KV write + logits."""
    H, I, V, L = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"], cfg["num_layers"]
    D, Hq, Hkv = cfg["head_dim"], cfg["num_heads"], cfg["num_kv_heads"]
    lin = L * ((Hq + 2 * Hkv) * D * H + H * Hq * D + 2 * I * H + H * I)
    wbytes = lin * (1 if weight_format == "fp8" else 2)
    scales = (lin // (128 * 128)) * 2 if weight_format == "fp8" else 0
    norms = L * (2 * H + 2 * D) * 2 + H * 2
    lm = V * H * 2
    kv_row = L * 2 * Hkv * D * 2
    return {"weights": wbytes + scales + norms, "lm_head": lm, "kv_read": kv_row * ctx, "kv_write": kv_row,
            "logits": V * 4, "total": wbytes + scales + norms + lm + kv_row * ctx + kv_row + V * 4}


def kernel_bytes_per_launch(cfg: dict, ctx: int, B: int) -> dict:
    """Algorithmic bytes ONE launch of each decode-step kernel class moves (bf16 weights, batch B, context ctx):
    the weight matrix once, the fp32 activation vectors in and out once per sequence, K/V rows once per sequence.
    DESIGN.md 4.1 lists the same terms."""
    H, I, V = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"]
    D, Hq, Hkv = cfg["head_dim"], cfg["num_heads"], cfg["num_kv_heads"]
    nqkv, qd = (Hq + 2 * Hkv) * D, Hq * D
    kv = 2 * Hkv * D * 2                      # K + V bytes of one cached position of one layer
    return {
        "norm_qkv": nqkv * H * 2 + H * 2 + B * (H * 4 + nqkv * 4),
        # short-context fused kernel: W_o + the cached rows + the new row written + q/k/v in + Hkv partial vectors out
        "attn": H * qd * 2 + B * (kv * ctx + kv + nqkv * 4 + Hkv * H * 4),
        "oproj": H * qd * 2 + B * (qd * 4 + 2 * H * 4),
        "gateup": 2 * I * H * 2 + H * 2 + B * ((1 + Hkv) * H * 4 + I * 4),
        "down": H * I * 2 + B * (I * 4 + 2 * H * 4),
        "lmhead": V * H * 2 + H * 2 + B * (H * 4 + V * 4),
        "argmax": B * (1024 * 8 + H * 2 + H * 4),
    }


def prefill_flops(cfg: dict, S: int, all_rows: bool) -> float:
    H, I, V, L = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"], cfg["num_layers"]
    D, Hq, Hkv = cfg["head_dim"], cfg["num_heads"], cfg["num_kv_heads"]
    per_tok = L * ((Hq + 2 * Hkv) * D * H + H * Hq * D + 3 * I * H)
    gemm = 2.0 * S * per_tok + 2.0 * (S if all_rows else 1) * V * H
    attn = 4.0 * S * S * D * Hq * L / 2
    return gemm + attn


def cpu_baseline(cfg, weights, prompt, n_decode: int) -> dict:
    """Reference-semantics NumPy path (oracle/cpu_ref.py == the reference's CPUSimulationBackend numerics,
    pinned by tests/golden) on this box's host cores: prefill the prompt, then time n_decode cached steps."""
    from oracle import cpu_ref as O

    try:
        from threadpoolctl import threadpool_info

        threads = max([p.get("num_threads", 1) for p in threadpool_info()] or [1])
    except Exception:
        threads = os.cpu_count() or 1
    ref = O.build_qwen3_ref(cfg, weights, max_pos=len(prompt) + n_decode + 8)
    t0 = time.perf_counter()
    hidden, past = ref(prompt, use_cache=True)
    nxt = int(np.argmax(ref.get_logits(hidden[-1:])[0]))
    t_prefill = time.perf_counter() - t0
    t0 = time.perf_counter()
    for _ in range(n_decode):
        hidden, past = ref([nxt], past_key_values=past, use_cache=True)
        nxt = int(np.argmax(ref.get_logits(hidden)[0]))
    dt = time.perf_counter() - t0
    return {"value": n_decode / dt, "unit": "tokens/s", "cores": int(threads), "kind": "port",
            "sample": f"NumPy oracle, fp32 on the same bf16-rounded weights: {len(prompt)}-token prefill "
                      f"({t_prefill:.1f} s) then {n_decode} cached decode steps ({dt:.1f} s)",
            "prefill_s": t_prefill}


DUMP_LOGITS_BYTES = 48 << 20     # the token log is small; everything dumped stays under 64 MB


def dump_outputs(out_dir: str, logits: np.ndarray, tokens: np.ndarray) -> None:
    """The headline path's outputs after the timed steps, as .npy files (see the module docstring)."""
    os.makedirs(out_dir, exist_ok=True)
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    if logits.nbytes > DUMP_LOGITS_BYTES:
        n = DUMP_LOGITS_BYTES // logits[0].nbytes
        rows = np.sort(np.random.default_rng(0).choice(logits.shape[0], n, replace=False))
        np.save(os.path.join(out_dir, "logits_rows.npy"), rows.astype(np.float64))
        logits = logits[rows]
    np.save(os.path.join(out_dir, "logits.npy"), logits)
    np.save(os.path.join(out_dir, "tokens.npy"), np.asarray(tokens, dtype=np.float64))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--batch-per-gpu", type=int, default=1, help="sequences per GPU of the HEADLINE leg (BASELINE config 2: 1)")
    ap.add_argument("--prompt-len", type=int, default=128)
    ap.add_argument("--max-seq-len", type=int, default=0,
                    help="KV-cache rows per sequence of the headline engine (default: prompt + warmup + steps + 8); the launch "
                         "sequence follows the CONTEXT, not this capacity")
    ap.add_argument("--weight-format", choices=["bf16", "fp8"], default="bf16")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--full", action="store_true",
                    help="after the headline (and the dump), also run every other leg: prefill timings, per-kernel roofline, "
                         "config 4, the extras, the CPU baseline (--cpu-decode-tokens, --no-cpu-baseline, --long-prefill, "
                         "--no-config5, --no-extras and --config4-steps shape those legs and do nothing without --full)")
    ap.add_argument("--cpu-decode-tokens", type=int, default=16)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--long-prefill", type=int, default=2048,
                    help="also time a prefill of this many tokens (the MFMA-bound regime); 0 = skip")
    ap.add_argument("--no-config5", action="store_true", help="skip the Llama-3-8B-shape fp8 prefill leg of 'extras' (~25 s)")
    ap.add_argument("--no-extras", action="store_true",
                    help="skip every extra leg (config 4 weak/strong; at N = 1 also context 2048 in bf16 and w8a16, config 5)")
    ap.add_argument("--config4-steps", type=int, default=32)
    ap.add_argument("--layers", type=int, default=0, help="debug only: override the layer count (result is then INVALID)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's logits and the token log as DIR/<name>.npy (float32 / float64)")
    args = ap.parse_args()

    # ONE JSON line on stdout, whatever the libraries underneath print: RCCL writes a version banner to the process's stdout
    # during communicator bring-up (seen in the two-rank rehearsal, profiles/r03_n2_rehearsal.txt).  File descriptor 1 is
    # pointed at stderr for the run; the result line goes to the saved descriptor.
    sys.stdout.flush()
    result_fd = os.dup(1)
    os.dup2(2, 1)

    def emit(obj) -> None:
        os.write(result_fd, (json.dumps(obj) + "\n").encode())

    from pygpukit_amd import _hip
    from pygpukit_amd.core.array import GPUArray
    from pygpukit_amd.core.dtypes import bfloat16, int32, uint8
    from pygpukit_amd.core.factory import from_numpy
    from pygpukit_amd.llm import synthetic as S
    from pygpukit_amd.llm.engine import Engine
    from pygpukit_amd import parallel as DP
    from pygpukit_amd.parallel import ControlPlane, RcclComm

    cp = ControlPlane()
    if cp.world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={cp.world}: launch with torch.distributed.run --nproc-per-node {args.gpus}")
    ndev = _hip.device_count()
    my_device = cp.local_rank % max(ndev, 1)
    _hip.call("pgk_device_set", my_device)
    if os.environ.get("PGK_REHEARSE_SHARED_GPU") == "1":
        # rehearsal on a box with fewer GPUs than ranks (tools/rehearse_n2.sh): the ranks share devices, so the launcher
        # rendezvous, the RCCL id exchange and communicator bring-up (or its refusal of a duplicate GPU -> exit 3 on every
        # rank) run with real processes.  The number such a run prints is NOT a scaling measurement.
        ndev = max(ndev, cp.world)
    # RCCL carries the one-time weight broadcast and the end-of-run token gather.  For N > 1 it is mandatory: a run
    # whose communicator does not come up prints the reason and exits non-zero instead of reporting a number that no
    # RCCL traffic stands behind (parallel.open_comm: every rank takes the same branch).
    try:
        comm = DP.open_comm(cp, ndev, lambda cp_: RcclComm(cp_, device=my_device))
    except DP.CommUnavailable as e:
        if cp.rank == 0:
            emit({"error": "RCCL is mandatory for --gpus > 1 and did not come up", "detail": str(e), "n_gpus": cp.world})
        cp.shutdown()
        raise SystemExit(3)

    start_ev, stop_ev = _hip.C.c_void_p(), _hip.C.c_void_p()
    _hip.call("pgk_event_create", _hip.C.byref(start_ev))
    _hip.call("pgk_event_create", _hip.C.byref(stop_ev))

    class GpuOps:
        """parallel.py's `ops` protocol on the device: GPUArrays, hipEvents on the default stream."""
        @staticmethod
        def sync():
            _hip.call("pgk_device_sync")

        @staticmethod
        def empty(shape, dt):
            return GPUArray(tuple(shape), {np.dtype(np.int32): int32}[np.dtype(dt)])

        from_host = staticmethod(from_numpy)

        @staticmethod
        def to_host(arr):
            return arr.to_numpy()

        @staticmethod
        def nbytes(arr):
            return arr.nbytes

        @staticmethod
        def timer_start():
            _hip.call("pgk_event_record", start_ev, None)

        @staticmethod
        def timer_stop_ms():
            _hip.call("pgk_event_record", stop_ev, None)
            _hip.call("pgk_event_sync", stop_ev)
            ms = _hip.C.c_float()
            _hip.call("pgk_event_elapsed_ms", start_ev, stop_ev, _hip.C.byref(ms))
            return ms.value

    ops = GpuOps()

    cfg = dict(S.QWEN3_0_6B)
    if args.layers:
        cfg["num_layers"] = args.layers
    B, K, W, P = args.batch_per_gpu, args.steps, args.warmup, args.prompt_len
    max_seq = max(args.max_seq_len, P + W + K + 8)
    t_setup = time.perf_counter()

    # ---- weights on the device: rank 0 draws them, every other rank receives them over RCCL (xGMI broadcast) ----
    weights = S.make_qwen3_weights(cfg, seed=args.seed) if cp.rank == 0 else None
    H, I, V, D = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"], cfg["head_dim"]
    nq = (cfg["num_heads"] + 2 * cfg["num_kv_heads"]) * D
    fp8 = args.weight_format == "fp8"
    wdt = uint8 if fp8 else bfloat16
    shapes = {"attn_norm": ((H,), bfloat16), "mlp_norm": ((H,), bfloat16), "q_norm": ((D,), bfloat16), "k_norm": ((D,), bfloat16),
              "w_qkv": ((nq, H), wdt), "w_o": ((H, cfg["num_heads"] * D), wdt), "w_gate_up": ((2 * I, H), wdt), "w_down": ((H, I), wdt)}
    if fp8:
        shapes.update({"s_qkv": ((nq // 128, H // 128), bfloat16), "s_o": ((H // 128, cfg["num_heads"] * D // 128), bfloat16),
                       "s_gate_up": ((2 * I // 128, H // 128), bfloat16), "s_down": ((H // 128, I // 128), bfloat16)})
    if cp.rank == 0:
        embed = S._bf16(weights["embed"])
        fnorm = S._bf16(weights["final_norm"])
        layers = [S.engine_layer_arrays(lw, args.weight_format) for lw in weights["layers"]]
    else:
        embed, fnorm = GPUArray((V, H), bfloat16), GPUArray((H,), bfloat16)
        layers = [{k: GPUArray(s, dt) for k, (s, dt) in shapes.items()} for _ in range(cfg["num_layers"])]
    bcast = DP.broadcast_weights(cp, comm, [embed, fnorm] + [lw[k] for lw in layers for k in shapes], ops)

    def new_engine(max_seq_len, max_batch):
        return Engine(cfg, embed, layers, fnorm, None, max_seq_len=max_seq_len, max_batch=max_batch, weight_format=args.weight_format)

    eng = new_engine(max_seq, B)

    # ---- prompts: one independent sequence per (rank, slot) ----
    rng = np.random.default_rng(1000 + args.seed)
    all_prompts = rng.integers(0, cfg["vocab_size"], (cp.world * B, P))
    mine = all_prompts[cp.rank * B:(cp.rank + 1) * B]

    # ---- prefill (MFMA path), timed on sequence slot 0 ----
    def timed_ms(fn, reps):
        out = []
        for _ in range(reps):
            _hip.call("pgk_event_record", start_ev, None)
            fn()
            _hip.call("pgk_event_record", stop_ev, None)
            _hip.call("pgk_event_sync", stop_ev)
            ms = _hip.C.c_float()
            _hip.call("pgk_event_elapsed_ms", start_ev, stop_ev, _hip.C.byref(ms))
            out.append(ms.value)
        return out

    # ---- headline: whole-step hipGraph, state in device memory; every rank's token log gathered once after the timed steps ----
    head = DP.headline_leg(cp, comm, eng, mine, ops, batch=B, prompt_len=P, warm=W, steps=K)
    wall_max, dev_ms_max, tokens, gather = head["wall_s"], head["device_ms"], head["tokens"], head["gather"]
    if gather is not None:
        gather.pop("all_tokens")
    if args.dump_outputs and cp.rank == 0:
        dump_outputs(args.dump_outputs, eng.logits(B).to_numpy(), tokens)

    # ---- whole-step roofline: arithmetic on the headline's own device time, no run of its own ----
    ctx_mid = P + W + K // 2
    ab = algorithmic_bytes_per_token(cfg, ctx_mid, args.weight_format)
    step_ms = dev_ms_max / K
    step_bytes = ab["weights"] + ab["lm_head"] + B * (ab["kv_read"] + ab["kv_write"] + ab["logits"])
    step_roofline = {"bound": "hbm", "achieved": step_bytes / (step_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": step_bytes / (step_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "bytes_per_step": step_bytes,
                     "launches_per_step": eng.launches_per_step(), "ctx_mid": ctx_mid, "step_us": step_ms * 1e3}

    result = {
        "metric": "decode tokens/sec/GPU + prefill TFLOPS (% MFMA peak), Qwen3-0.6B bf16",
        "value": cp.world * B * K / wall_max, "unit": "tokens/s", "n_gpus": cp.world, "steps": K, "warmup": W,
        "ms_per_step": wall_max * 1e3 / K, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "bf16" if args.weight_format == "bf16" else "fp8-e4m3 weights x bf16", "data": "synthetic",
        "config": {"workload": f"Qwen3-0.6B-shape random-init {args.weight_format}, prefill {P} + {K}-token greedy decode, "
                               f"whole-step hipGraph, {B} sequence(s) per GPU (BASELINE config 2{'' if cp.world == 1 else ' on every GPU: data-parallel replicas'})",
                   "batch_per_gpu": B, "global_batch": cp.world * B, "prompt_len": P, "parallelism": f"dp{cp.world}",
                   "layers": cfg["num_layers"], "max_seq_len": max_seq},
        "full": args.full, "tokens_per_s_per_gpu": B * K / wall_max, "device_ms_per_step": step_ms, "step_roofline": step_roofline,
        "first_tokens": [int(t) for t in tokens[: min(8, len(tokens)), 0]],
    }
    if gather is not None:
        result["token_gather"] = gather
    if bcast is not None:
        result["weight_broadcast"] = bcast
    if args.layers:
        result["INVALID"] = "layer count overridden"
    if args.full:
        result.update(full_legs(args, cp, cfg, eng, new_engine, weights, mine, ops, timed_ms, step_roofline))
    result["setup_s"] = time.perf_counter() - t_setup
    if args.full and cp.rank == 0 and cp.world == 1 and not args.no_cpu_baseline:
        del eng
        result["cpu_baseline"] = cpu_baseline(cfg, weights, [int(t) for t in mine[0]], args.cpu_decode_tokens)
    elif args.full and cp.rank == 0:
        result["cpu_baseline"] = None
    if cp.rank == 0:
        emit(result)
    cp.barrier()
    if comm is not None:
        comm.destroy()
    cp.shutdown()


def full_legs(args, cp, cfg, eng, new_engine, weights, mine, ops, timed_ms, step_roofline) -> dict:
    """Everything `--full` measures beyond the headline, on the headline's engine and weights after its steps and its dump:
    the 128-token prefill, the per-kernel roofline, config 4 and the other extras, the long prefill.  Returns the
    result line's additional objects; fills `step_roofline["sum_of_kernel_us"]`."""
    from pygpukit_amd import _hip
    from pygpukit_amd import parallel as DP
    from pygpukit_amd.llm import synthetic as S
    from pygpukit_amd.llm.engine import Engine

    B, K, W, P = args.batch_per_gpu, args.steps, args.warmup, args.prompt_len
    pf_ms = timed_ms(lambda: eng.prefill([int(t) for t in mine[0]], seq=0, want_last_logits=False), 5)    # slot 0's rows are rewritten with the same values
    pf_med = float(np.median(pf_ms))
    pf_flops = prefill_flops(cfg, P, all_rows=False)

    # ---- per-kernel timing: eager steps, start/stop events on every launch (rank 0's numbers are reported) ----
    prof = eng.profile_step(B, 8)
    ctx_mid = P + W + K // 2
    rows = []
    kb = kernel_bytes_per_launch(cfg, ctx_mid, B)
    NAMES = {"norm_qkv": "fused_gemv_kernel<PRO_NORM, EPI_STORE> (RMSNorm + qkv projection)",
             "attn": "attn_oproj_mfma_kernel (QK-norm, RoPE, KV write, attention on MFMA from LDS-staged K/V, o_proj partials; attn_oproj_kernel when head_dim != 128)",
             "oproj": "fused_gemv_kernel<PRO_PLAIN, EPI_RESID> (o_proj + residual)",
             "gateup": "fused_gemv_kernel<PRO_NORM_SUM, EPI_SWIGLU> (residual sum + RMSNorm + gate/up + SwiGLU)",
             "down": "fused_gemv_kernel<PRO_PLAIN, EPI_RESID> (down projection + residual)",
             "lmhead": "fused_gemv_kernel<PRO_NORM, EPI_LOGITS> (final norm + lm_head + argmax partials)",
             "argmax": "finalize_kernel (argmax, position, token log, next embedding row)"}
    total_us = sum(us * n for us, n in prof.values())
    for k, (us, n) in prof.items():
        if not n or k not in kb:
            continue
        by = kb[k] if (B == 1 and args.weight_format == "bf16") else None
        row = {"kernel": NAMES.get(k, k), "class": k, "launches_per_step": n, "us_per_launch": us,
               "share_of_step_kernel_time": us * n / total_us if total_us else None, "bound": "hbm",
               "bytes_per_launch": by, "achieved": by / us / 1e3 if (by and us) else None, "peak": HBM_PEAK_GBS, "unit": "GB/s",
               "frac": by / us / 1e3 / HBM_PEAK_GBS if (by and us) else None, "traffic": None}
        rows.append(row)
    rows.sort(key=lambda r: -(r["share_of_step_kernel_time"] or 0))
    roofline = dict(rows[0]) if rows else None
    if roofline:
        roofline["timing"] = ("start/stop hipEvents on every launch (hipExtLaunchKernelGGL, the launch stream) of 8 eager steps: "
                              "dispatch begin -> end, the interval rocprofv3 --kernel-trace reports; nothing subtracted")
    step_roofline["sum_of_kernel_us"] = total_us

    extras = None
    if not args.no_extras and B == 1 and args.weight_format == "bf16" and P == 128:
        extras = {}
        # ---- BASELINE config 4 at this N: weak (8 per GPU) and strong (64 / N per GPU); parallel.config4_legs ----
        def bytes4(b_local):
            ab4 = algorithmic_bytes_per_token(cfg, P + 4 + args.config4_steps // 2, "bf16")
            return ab4["weights"] + ab4["lm_head"] + b_local * (ab4["kv_read"] + ab4["kv_write"] + ab4["logits"])
        extras["config4"] = DP.config4_legs(cp, new_engine, lambda n, plen: np.random.default_rng(3000 + args.seed).integers(0, cfg["vocab_size"], (n, plen)),
                                            ops, prompt_len=P, steps=args.config4_steps, warm=4, bytes_per_step=bytes4, hbm_peak_gbs=HBM_PEAK_GBS)

    # ---- single-GPU-only legs ----
    long_pf = None
    if args.long_prefill > 0 and cp.world == 1:
        SL = args.long_prefill
        eng_l = new_engine(SL + 8, 1)   # same device weights, its own KV cache
        lp = [int(t) for t in np.random.default_rng(2000 + args.seed).integers(0, cfg["vocab_size"], SL)]
        eng_l.prefill(lp, want_last_logits=False)
        l_ms = timed_ms(lambda: eng_l.prefill(lp, want_last_logits=False), 3)
        lf = prefill_flops(cfg, SL, all_rows=False)
        lmed = float(np.median(l_ms))
        long_pf = {"tokens": SL, "ms": lmed, "tflops": lf / (lmed * 1e-3) / 1e12, "flops": lf, "logits": "last row only",
                   "frac_mfma_peak": lf / (lmed * 1e-3) / 1e12 / MFMA_BF16_PEAK_TFLOPS, "tokens_per_s": SL / (lmed * 1e-3),
                   "runs_ms": [round(x, 3) for x in l_ms]}
        del eng_l

    if extras is not None and cp.world == 1:
        def ctx_leg(fmt, batch, prompt_len, steps=32, warm=4):
            e2 = S.build_engine_from_weights(cfg, weights, max_seq_len=prompt_len + steps + warm + 8, max_batch=batch, weight_format=fmt)
            pr = np.random.default_rng(3000 + args.seed).integers(0, cfg["vocab_size"], (batch, prompt_len))
            f0 = [int(np.argmax(e2.prefill([int(t) for t in pr[b]], seq=b))) for b in range(batch)]
            e2.set_state(f0, [prompt_len] * batch)
            e2.capture(batch)
            e2.replay(warm)
            _hip.call("pgk_device_sync")
            t0 = time.perf_counter()
            e2.replay(steps)
            _hip.call("pgk_device_sync")
            dt = time.perf_counter() - t0
            ab2 = algorithmic_bytes_per_token(cfg, prompt_len + warm + steps // 2, fmt)
            by = ab2["weights"] + ab2["lm_head"] + batch * (ab2["kv_read"] + ab2["kv_write"] + ab2["logits"])
            return {"tokens_per_s": batch * steps / dt, "ms_per_step": dt * 1e3 / steps, "batch": batch, "context": prompt_len,
                    "weights": fmt, "hbm_frac": by / (dt / steps) / 1e9 / HBM_PEAK_GBS}
        extras["config3_ctx2048_w8a16"] = ctx_leg("fp8", 1, 2048)
        extras["ctx2048_bf16"] = ctx_leg("bf16", 1, 2048)

        def config5_leg(S_tok=4096, reps=3):
            """BASELINE config 5: Llama-3-8B-shape random-init weights, fp8 e4m3 x fp8 MFMA prefill of 4096 tokens (and the
            bf16 prefill of the same model beside it).  FLOPs: projection GEMMs + causal attention + last-row lm_head."""
            c5 = dict(S.LLAMA3_8B)
            w5 = S.random_engine_weights(c5, seed=args.seed, fp8=True, keep_bf16=True, threads=12)
            H5, D5, I5, V5, L5 = c5["hidden_size"], c5["head_dim"], c5["intermediate_size"], c5["vocab_size"], c5["num_layers"]
            per_layer = H5 * (c5["num_heads"] + 2 * c5["num_kv_heads"]) * D5 + c5["num_heads"] * D5 * H5 + 3 * H5 * I5
            flops = 2.0 * S_tok * L5 * per_layer + 2.0 * V5 * H5 + 4.0 * S_tok * S_tok * D5 * c5["num_heads"] * L5 / 2
            toks = [int(t) for t in np.random.default_rng(4000 + args.seed).integers(0, V5, S_tok)]
            out = {"tokens": S_tok, "layers": L5, "flops": flops,
                   "parity": "BASELINE's 5e-2 end-to-end bar (fp8 vs bf16 logits) is NOT met on random-init weights at 32 layers "
                             "(e4m3 quantisation itself, oracle included); it is met per GEMM: DESIGN.md 4.3, profiles/r02_config5_depth_error.json"}
            for fmt, peak in (("fp8a8", 2 * MFMA_BF16_PEAK_TFLOPS), ("bf16", MFMA_BF16_PEAK_TFLOPS)):
                e5 = Engine(c5, w5["embed"], w5["bf16"] if fmt == "bf16" else w5["fp8"], w5["final_norm"], None, max_seq_len=S_tok + 8,
                            max_batch=1, weight_format=fmt, use_qk_norm=False)
                e5.prefill(toks, want_last_logits=False)
                e5.synchronize()
                ms = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    e5.prefill(toks, want_last_logits=False)
                    e5.synchronize()
                    ms.append((time.perf_counter() - t0) * 1e3)
                best = min(ms)
                out[fmt] = {"ms": best, "tflops": flops / best / 1e9, "frac_mfma_peak": flops / best / 1e9 / peak,
                            "peak_tflops": peak, "runs_ms": [round(x, 2) for x in ms]}
                del e5
            return out

        if not args.no_config5:
            try:
                extras["config5_llama8b_prefill4096"] = config5_leg()
            except Exception as e:  # noqa: BLE001 - an extra leg must never take the headline down
                extras["config5_llama8b_prefill4096"] = {"error": f"{type(e).__name__}: {e}"}

    return {"roofline": roofline, "roofline_kernels": rows,
            "prefill": {"ms": pf_med, "tflops": pf_flops / (pf_med * 1e-3) / 1e12, "flops": pf_flops, "logits": "last row only",
                        "frac_mfma_peak": pf_flops / (pf_med * 1e-3) / 1e12 / MFMA_BF16_PEAK_TFLOPS, "runs_ms": [round(x, 3) for x in pf_ms]},
            "prefill_long": long_pf, "extras": extras}


if __name__ == "__main__":
    main()
