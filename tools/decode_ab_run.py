"""One run of the batch-1 decode A/B protocol: a fresh process builds the engine (Qwen3-0.6B bf16, cache
208), times 7 windows of 64 replayed steps from context 128 and prints one JSON line with the median ms per step.
    PGK_LIB=<library> python tools/decode_ab_run.py <label>
Optional: --start P (first timed position, = prompt length), --steps N (per window), --cache ROWS, --windows W, and
--fixed P1,P2,...: fixed-context mode - one engine, per listed position 7 windows of N steps that ALL run at that position
(set_state before every replayed step, one synchronize per window; the state upload is inside the time, alike at every
position, so differences between positions are the kernels').  One JSON line per position."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pygpukit_amd.llm import synthetic as S
ap = argparse.ArgumentParser()
ap.add_argument("label", nargs="?", default="run")
ap.add_argument("--start", type=int, default=128)
ap.add_argument("--steps", type=int, default=64)
ap.add_argument("--cache", type=int, default=208)
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--fixed", type=str, default="")
args = ap.parse_args()
label, P, STEPS, WINDOWS = args.label, args.start, args.steps, args.windows
fixed = [int(p) for p in args.fixed.split(",") if p]
cfg = dict(S.QWEN3_0_6B)
w = S.make_qwen3_weights(cfg, seed=0)
eng = S.build_engine_from_weights(cfg, w, max_seq_len=args.cache, max_batch=1)
if fixed:
    P = max(fixed)
pr = [int(t) for t in np.random.default_rng(1).integers(0, cfg["vocab_size"], P)]
first = int(np.argmax(eng.prefill(pr)))
if fixed:
    order = fixed if label.encode()[-1] % 2 else fixed[::-1]      # runs alternate the order of the positions with their label
    for p in order:
        eng.set_state([first], [p])
        eng.capture(1)
        ms = []
        for i in range(WINDOWS + 1):                  # window 0 warms up
            eng.synchronize()
            t0 = time.perf_counter()
            for _ in range(STEPS):
                eng.set_state([first], [p])
                eng.replay(1)
            eng.synchronize(); dt = time.perf_counter() - t0
            if i:
                ms.append(dt * 1e3 / STEPS)
        print(json.dumps({"build": label, "fixed_position": p, "cache": args.cache, "ms_step_median": round(float(np.median(ms)), 5),
                          "ms_step_windows": [round(m, 5) for m in ms], "launches": eng.launches_per_step()}), flush=True)
    sys.exit(0)
eng.set_state([first], [P])
eng.capture(1)
ms = []
for i in range(WINDOWS + 1):                      # window 0 warms up
    eng.set_state([first], [P])
    eng.synchronize()
    t0 = time.perf_counter(); eng.replay(STEPS); eng.synchronize(); dt = time.perf_counter() - t0
    if i:
        ms.append(dt * 1e3 / STEPS)
print(json.dumps({"build": label, "ms_step_median": round(float(np.median(ms)), 5), "ms_step_windows": [round(m, 5) for m in ms],
                  "last_token": int(eng.read_tokens(1, 1)[0][0]), "launches": eng.launches_per_step()}))
