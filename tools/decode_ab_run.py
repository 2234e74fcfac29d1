"""One run of the batch-1 decode A/B protocol: a fresh process builds the engine (Qwen3-0.6B bf16, cache
208), times 7 windows of 64 replayed steps from context 128 and prints one JSON line with the median ms per step.
    PGK_LIB=<library> python tools/decode_ab_run.py <label>"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pygpukit_amd.llm import synthetic as S
label = sys.argv[1] if len(sys.argv) > 1 else "run"
P, STEPS, WINDOWS = 128, 64, 7
cfg = dict(S.QWEN3_0_6B)
w = S.make_qwen3_weights(cfg, seed=0)
eng = S.build_engine_from_weights(cfg, w, max_seq_len=208, max_batch=1)
pr = [int(t) for t in np.random.default_rng(1).integers(0, cfg["vocab_size"], P)]
first = int(np.argmax(eng.prefill(pr)))
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
