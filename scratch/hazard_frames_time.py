#!/usr/bin/env python3
"""Wall time of the moving-hazard calls at 4096 robots x 1000 steps, doggo 2x64 (profiles/r13/hazard_frames.txt).

  python scratch/hazard_frames_time.py PARENT_TREE   (a source tree of the parent commit with its built mobrob_amd/libmobrob_ppo.so)
(a) existing calls -- evaluate / follow, plain and with static hazards (M = 16 and 256, shared scene) -- on the parent tree and
    on this one, alternating parent / this / parent / this, --runs timed calls after --warmup each: the spread of each library.
(b) new calls on this tree: evaluate / follow with a MovingHazards against the static call at the same M in the same process:
    shared scene M = 16 and 256 with frame_steps = 50 (F = 20: 19 restages in 1000 steps) and frame_steps = 1 (F = 1000: a restage
    every step); per-robot scenes M = 16 with frame_steps = 50 (F = 20) and frame_steps = 1 (F = 20, loop: the same 15 MiB table;
    the 64 MiB cap allows 85 frames of 4096 x 16 hazards).  Hazards uniform in the arena in every frame, radius 0.3, shaped cost.
Calls are synchronous (they return after the copy-out).  Each leg runs in a child process of its own, importing the package from
its tree.

Every leg is timed on three clocks: time.perf_counter per call (the figures reported), and over the whole batch of timed calls
time.time and a pair of HIP events (the device's own clock, through the HIP runtime the engine's library loaded -- torch is not
imported: a second HIP runtime brought up after the engine's found no device; the calls are synchronous, so the events bracket
the same work).  A leg whose three batch totals differ by more than 5 % is flagged CLOCKS DISAGREE and its figures are not to
be used; the plain calls double as an anchor against profiles/r9/hazards.txt (evaluate 6.37 ms, follow 6.77 ms on the same GPU)."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("HAZARD_TIME_TREE", ROOT))
N, STEPS = 4096, 1000


def setup():
    from mobrob_amd.engine import PPOEngine
    from mobrob_amd.envs.vec_env import DeviceGoalVecEnv
    from oracle import ppo_oracle as O
    e = PPOEngine(obs_dim=58, act_dim=12, n_envs=16, n_steps=16, batch_size=64, n_epochs=1, pi=(64, 64), vf=(64, 64), seed=1)
    e.set_params(O.init_params(58, 12, (64, 64), (64, 64), seed=0))
    env = DeviceGoalVecEnv.for_robot("doggo", N, time_limit=0)
    square = 2.5 * np.array([[1.0, 1.0], [1.0, -1.0], [-1.0, -1.0], [-1.0, 1.0]], np.float32)
    start = np.random.default_rng(0).uniform(-0.5, 0.5, (N, 2)).astype(np.float32)
    return e, env, square, start


_HIP = None


def _hip():
    """the HIP runtime the engine's library already loaded (no second runtime in the process): hipEvent* through ctypes"""
    global _HIP
    if _HIP is None:
        import ctypes
        with open("/proc/self/maps") as f:                 # the copy mapped by libmobrob_ppo.so, by its path
            paths = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})
        if len(paths) != 1:
            raise RuntimeError(f"expected one HIP runtime in the process, found {paths}")
        _HIP = ctypes.CDLL(paths[0])
        _HIP.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
        _HIP.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        _HIP.hipEventSynchronize.argtypes = [ctypes.c_void_p]
    return _HIP


def _hip_ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: HIP error {rc}")


def times(fn, runs, warmup):
    """-> {"t": per-call perf_counter seconds, "wall": batch seconds by time.time, "gpu": batch seconds by HIP events}"""
    import ctypes
    hip = _hip()
    for _ in range(warmup):
        fn()
    ev0, ev1 = ctypes.c_void_p(), ctypes.c_void_p()
    _hip_ok(hip.hipEventCreate(ctypes.byref(ev0)), "hipEventCreate")
    _hip_ok(hip.hipEventCreate(ctypes.byref(ev1)), "hipEventCreate")
    ts = []
    w0 = time.time()
    _hip_ok(hip.hipEventRecord(ev0, None), "hipEventRecord")
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    _hip_ok(hip.hipEventRecord(ev1, None), "hipEventRecord")
    _hip_ok(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
    wall = time.time() - w0
    ms = ctypes.c_float()
    _hip_ok(hip.hipEventElapsedTime(ctypes.byref(ms), ev0, ev1), "hipEventElapsedTime")
    hip.hipEventDestroy(ev0)
    hip.hipEventDestroy(ev1)
    return {"t": ts, "wall": wall, "gpu": ms.value * 1e-3}


def static_scene(M, S, rng):
    from mobrob_amd.envs.goal_rules import Hazards
    if S == 1:
        return Hazards(rng.uniform(-3, 3, (M, 2)), 0.3, indicator=False)
    return Hazards(rng.uniform(-3, 3, (S, M, 2)), 0.3, indicator=False, scene=np.arange(N))


def leg_existing(runs, warmup):
    e, env, square, start = setup()
    out = {"evaluate": times(lambda: env.evaluate(e, n_robots=N, max_steps=STEPS, seed=1), runs, warmup),
           "follow": times(lambda: env.follow(e, start, square, max_steps=STEPS, seed=1), runs, warmup)}
    rng = np.random.default_rng(3)
    for M in (16, 256):
        hz = static_scene(M, 1, rng)
        out[f"evaluate M={M}"] = times(lambda: env.evaluate(e, n_robots=N, max_steps=STEPS, seed=1, hazards=hz), runs, warmup)
        out[f"follow M={M}"] = times(lambda: env.follow(e, start, square, max_steps=STEPS, seed=1, hazards=hz), runs, warmup)
    return out


FRAME_LEGS = [(16, 1, 50, 20, False), (16, 1, 1, 1000, False), (256, 1, 50, 20, False), (256, 1, 1, 1000, False),
              (16, N, 50, 20, False), (16, N, 1, 20, True)]           # M, S, frame_steps, F, loop


def leg_frames(runs, warmup):
    from mobrob_amd.envs.goal_rules import MovingHazards
    e, env, square, start = setup()
    rng = np.random.default_rng(3)
    out = {}
    for M, S in ((16, 1), (256, 1), (16, N)):
        hz = static_scene(M, S, rng)
        out[f"evaluate static M={M} S={S}"] = times(lambda: env.evaluate(e, n_robots=N, max_steps=STEPS, seed=1, hazards=hz), runs, warmup)
        out[f"follow static M={M} S={S}"] = times(lambda: env.follow(e, start, square, max_steps=STEPS, seed=1, hazards=hz), runs, warmup)
    for M, S, fs, F, loop in FRAME_LEGS:
        loc = rng.uniform(-3, 3, (F, M, 2) if S == 1 else (S, F, M, 2))
        mv = MovingHazards(loc, 0.3, frame_steps=fs, loop=loop, indicator=False, scene=None if S == 1 else np.arange(N))
        r = env.follow(e, start, square, max_steps=STEPS, seed=1, hazards=mv)
        assert r["persistent"]
        key = f"M={M} S={S} fs={fs} F={F}"
        out[f"evaluate {key}"] = times(lambda: env.evaluate(e, n_robots=N, max_steps=STEPS, seed=1, hazards=mv), runs, warmup)
        out[f"follow {key}"] = times(lambda: env.follow(e, start, square, max_steps=STEPS, seed=1, hazards=mv), runs, warmup)
        out[f"viol {key}"] = float(np.mean(r["violation_steps"] > 0))
    return out


def child(what, tree, runs, warmup):
    env = dict(os.environ, HAZARD_TIME_TREE=os.path.abspath(tree))
    for k in ("MOBROB_EVAL_PERSISTENT", "MOBROB_PPO_LIB"):
        env.pop(k, None)
    c = subprocess.run([sys.executable, __file__, "--leg", what, str(runs), str(warmup)], capture_output=True, text=True, env=env,
                       timeout=600)
    if c.returncode != 0:
        sys.exit(f"{what} {tree}: exit status {c.returncode}\n{c.stderr[-3000:]}")
    return json.loads(c.stdout.strip().splitlines()[-1])


def clocks(rec):
    """'ok' when the batch totals of the three clocks agree within 5 %, else what they say"""
    a = [sum(rec["t"]), rec["wall"], rec["gpu"]]
    return "ok" if max(a) <= 1.05 * min(a) else f"CLOCKS DISAGREE perf_counter {a[0]:.4f} s, time.time {a[1]:.4f} s, HIP events {a[2]:.4f} s"


def main():
    old, runs, warmup = sys.argv[1], 5, 2
    print(f"{N} robots x {STEPS} steps, doggo 2x64, persistent tile; synchronous calls; ms")
    keys = ["evaluate", "follow", "evaluate M=16", "follow M=16", "evaluate M=256", "follow M=256"]
    agg = {t: {k: [] for k in keys} for t in (old, ROOT)}
    flags = []
    for tree in (old, ROOT, old, ROOT):
        r = child("existing", tree, runs, warmup)
        for k in keys:
            agg[tree][k] += r[k]["t"]
            flags.append(clocks(r[k]))
    print(f"(a) existing calls, two alternating children per library, {runs} runs after {warmup} warm-up each: min / median / max")
    for k in keys:
        for tag, tree in (("parent", old), ("branch", ROOT)):
            t = 1e3 * np.array(agg[tree][k])
            print(f"  {k:<15} {tag}  {t.min():8.2f} {np.median(t):8.2f} {t.max():8.2f}")
    h = child("frames", ROOT, runs, warmup)
    print("(b) moving hazards (branch): median ms, ratio to the static call at the same M and S in the same process, violation rate")
    for M, S, fs, F, loop in FRAME_LEGS:
        key = f"M={M} S={S} fs={fs} F={F}"
        for k in ("evaluate", "follow"):
            base, rec = h[f"{k} static M={M} S={S}"], h[f"{k} {key}"]
            b, m = float(np.median(base["t"])), float(np.median(rec["t"]))
            flags += [clocks(base), clocks(rec)]
            print(f"  {k:<9} {key:<28}{' loop' if loop else '     '} {1e3 * m:8.2f} ms  static {1e3 * b:7.2f} ms  x{m / b:.3f}  "
                  f"+{1e3 * (m - b):.2f} ms  violation rate {h[f'viol {key}']:.3f}")
    bad = [f for f in flags if f != "ok"]
    print(f"clocks: {len(flags) - len(bad)} of {len(flags)} legs agree within 5 % on perf_counter, time.time and HIP events")
    for f in bad[:8]:
        print("  " + f)


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--leg":
        fn = leg_existing if sys.argv[2] == "existing" else leg_frames
        print(json.dumps(fn(int(sys.argv[3]), int(sys.argv[4]))))
    else:
        main()
