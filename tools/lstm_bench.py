"""Time pgk_lstm (bidirectional, B = 1, I = 512) on both recurrence paths in one process, alternating windows: per round
default (A), PGK_LSTM_RESIDENT=0, default again (A'), default with I = 8, stepped as a replayed hipGraph; N calls each between
device events after a warm-up of all of them.  Prints per shape and dtype the median us per call and per timestep of
  default   the path pgk_lstm_plan picks (resident for H <= 128, stepped above),
  stepped   PGK_LSTM_RESIDENT=0, eager: S + 2 launches enqueued by the host per call,
  graph     the same S + 2 launches captured once and replayed (what is left when the host is out of the way),
the spread of the default call against itself (A' / A and min..max of its windows: the margin inside which two numbers are
"the same"), and the projection's share: (t(I = 512) - t(I = 8)) / t(I = 512) of the default call - the part of the gate
projection that grows with I; its launch and the write of G stay in both and are not counted.
The yardstick for a stepped timestep is the box's dependent-launch floor: build and run tools/launch_floor.hip in the same
session.
usage: lstm_bench.py [--rounds N] [H S ...]      default: 64 128  64 512  128 128  128 512  256 128  256 512"""
import ctypes as C, os, statistics, sys, numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from pygpukit_amd import _hip
PGK = {"float32": 1, "bfloat16": 3}      # pgk_dtype, include/pgk_hip.h
B, I, I_SMALL = 1, 512, 8
DEFAULT = "64 128 64 512 128 128 128 512 256 128 256 512".split()


def dev(arr):
    p = C.c_void_p(); _hip.call("pgk_malloc", C.byref(p), max(arr.nbytes, 16))
    _hip.call("pgk_memcpy_h2d", p, arr.ctypes.data_as(C.c_void_p), arr.nbytes, None); return p


def words(a, dt):
    a = a.astype(np.float32)
    return a if dt == "float32" else (a.view(np.uint32) >> 16).astype(np.uint16)


def setup(H, S, isz, dt):
    """-> run(stream): one bidirectional pgk_lstm call on fixed buffers."""
    rng = np.random.default_rng(0)
    x = dev(words(rng.standard_normal((B, S, isz)), dt))
    dirs = []
    for _ in range(2):
        w = [rng.uniform(-1, 1, (4 * H, isz)) * 2 / np.sqrt(isz), rng.uniform(-1, 1, (4 * H, H)) * 2 / np.sqrt(H),
             rng.uniform(-.5, .5, 4 * H), rng.uniform(-.5, .5, 4 * H)]
        dirs.append(_hip.LstmDir(*[dev(words(a, dt)).value for a in w], None, None))
    es = 4 if dt == "float32" else 2
    out, hn, cn, gates, state = (dev(np.zeros(n, np.uint8)) for n in (B * S * 2 * H * es, 2 * B * H * es, 2 * B * H * es,
                                                                     2 * B * S * 4 * H * 4, 3 * 2 * B * H * 4))
    return lambda st=None: _hip.call("pgk_lstm", x, C.byref(dirs[0]), C.byref(dirs[1]), out, hn, cn, gates, state, B, S, isz, H, 0,
                                     PGK[dt], st)


def with_env(run, value):
    def f(st=None):
        if value is None: os.environ.pop("PGK_LSTM_RESIDENT", None)
        else: os.environ["PGK_LSTM_RESIDENT"] = value
        run(st)
    return f


def window_us(run, e0, e1, st, n):
    _hip.call("pgk_event_record", e0, st)
    for _ in range(n): run()
    _hip.call("pgk_event_record", e1, st); _hip.call("pgk_event_sync", e1)
    ms = C.c_float(); _hip.call("pgk_event_elapsed_ms", e0, e1, C.byref(ms))
    return ms.value * 1000 / n


def main():
    args = sys.argv[1:]
    rounds = 9
    if "--rounds" in args:
        i = args.index("--rounds"); rounds = int(args[i + 1]); del args[i:i + 2]
    a = args or DEFAULT
    _hip.require_device()
    e0, e1, gs = C.c_void_p(), C.c_void_p(), C.c_void_p()
    _hip.call("pgk_event_create", C.byref(e0)); _hip.call("pgk_event_create", C.byref(e1)); _hip.call("pgk_stream_create", C.byref(gs), 0)
    plan = _hip.load().pgk_lstm_plan
    for i in range(0, len(a), 2):
        H, S = int(a[i]), int(a[i + 1])
        n = 10 if S <= 128 else 4
        for dt in PGK:
            full, small = setup(H, S, I, dt), setup(H, S, I_SMALL, dt)
            default, stepped, default_small = with_env(full, None), with_env(full, "0"), with_env(small, None)
            os.environ.pop("PGK_LSTM_RESIDENT", None)
            path = "resident" if plan(B, H, PGK[dt]) else "stepped"
            # the stepped call as a graph: captured once on its own stream, replayed there
            os.environ["PGK_LSTM_RESIDENT"] = "0"
            g = C.c_void_p()
            _hip.call("pgk_graph_begin_capture", gs); full(gs); _hip.call("pgk_graph_end_capture", gs, C.byref(g))
            nodes = C.c_size_t(); _hip.call("pgk_graph_num_nodes", g, C.byref(nodes))
            replay = lambda: _hip.call("pgk_graph_launch", g, gs)
            for _ in range(3): default(); stepped(); default_small(); replay()
            _hip.call("pgk_device_sync")
            ta, ts, tb, tsm, tg = [], [], [], [], []
            for _ in range(rounds):
                ta.append(window_us(default, e0, e1, None, n)); ts.append(window_us(stepped, e0, e1, None, n))
                tb.append(window_us(default, e0, e1, None, n)); tsm.append(window_us(default_small, e0, e1, None, n))
                tg.append(window_us(replay, e0, e1, gs, n))
            _hip.call("pgk_device_sync"); _hip.call("pgk_graph_destroy", g)
            med = statistics.median
            md, ma, mb = med(ta + tb), med(ta), med(tb)
            print(f"BiLSTM B={B} I={I} H={H} S={S} {dt}, {rounds} rounds of {n} calls; default path: {path}")
            print(f"  default ({path:8s}) {md:9.1f} us/call {md / S:7.3f} us/step   (A {ma:.1f}, A' {mb:.1f}, A'/A {mb / ma:6.4f}, windows {min(ta + tb):.1f} .. {max(ta + tb):.1f} us)")
            print(f"  stepped, eager     {med(ts):9.1f} us/call {med(ts) / S:7.3f} us/step   (windows {min(ts):.1f} .. {max(ts):.1f} us)")
            print(f"  stepped, graph     {med(tg):9.1f} us/call {med(tg) / S:7.3f} us/step   ({nodes.value} nodes; windows {min(tg):.1f} .. {max(tg):.1f} us)")
            print(f"  default with I={I_SMALL}: {med(tsm):9.1f} us/call -> projection's I-dependent share {(md - med(tsm)) / md * 100:5.1f} %   default / stepped-eager {md / med(ts):6.3f}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
