#!/usr/bin/env python3
"""Wall time of the hazard-cost calls at 4096 robots x 1000 steps, doggo 2x64 (profiles/r9/hazards.txt).

  python scratch/hazard_time.py OLD_TREE NEW_TREE   (source trees with their built mobrob_amd/libmobrob_ppo.so)
(a) existing calls: evaluate_goal_env and follow_waypoints (persistent tile) on both trees, alternating old / new / old / new,
    --runs timed calls after --warmup each time: the spread of each library over all its runs.
(b) new calls on NEW.so: evaluate / follow with hazards at M = 0, 16, 256, 1024, one shared scene (S = 1, staged in LDS) and one
    scene per robot (S = n, read from global memory), hazards uniform in the arena, radius 0.3, shaped cost; median and the ratio
    to the same call without hazards measured in the same process.  Calls are synchronous (they return after the copy-out).
Each leg runs in a child process of its own, importing the package from its tree."""
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


def times(fn, runs, warmup):
    ts = []
    for i in range(warmup + runs):
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            ts.append(time.perf_counter() - t0)
    return ts


def leg_existing(runs, warmup):
    e, env, square, start = setup()
    return {"evaluate": times(lambda: env.evaluate(e, n_robots=N, max_steps=STEPS, seed=1), runs, warmup),
            "follow": times(lambda: env.follow(e, start, square, max_steps=STEPS, seed=1), runs, warmup)}


def leg_hazards(runs, warmup):
    from mobrob_amd.envs.goal_rules import Hazards
    e, env, square, start = setup()
    out = {"evaluate": times(lambda: env.evaluate(e, n_robots=N, max_steps=STEPS, seed=1), runs, warmup),
           "follow": times(lambda: env.follow(e, start, square, max_steps=STEPS, seed=1), runs, warmup)}
    rng = np.random.default_rng(3)
    for M in (0, 16, 256, 1024):
        for S in (1, N):
            if S == 1:
                hz = Hazards(rng.uniform(-3, 3, (M, 2)), 0.3, indicator=False)
            else:
                hz = Hazards(rng.uniform(-3, 3, (S, M, 2)), 0.3, indicator=False, scene=np.arange(N))
            r = env.follow(e, start, square, max_steps=STEPS, seed=1, hazards=hz)
            assert r["persistent"]
            out[f"evaluate M={M} S={S}"] = times(lambda: env.evaluate(e, n_robots=N, max_steps=STEPS, seed=1, hazards=hz), runs, warmup)
            out[f"follow M={M} S={S}"] = times(lambda: env.follow(e, start, square, max_steps=STEPS, seed=1, hazards=hz), runs, warmup)
            out[f"viol M={M} S={S}"] = [float(np.mean(r["violation_steps"] > 0))]
    return out


def child(what, tree, runs, warmup):
    env = dict(os.environ, HAZARD_TIME_TREE=os.path.abspath(tree))
    for k in ("MOBROB_EVAL_PERSISTENT", "MOBROB_PPO_LIB"):
        env.pop(k, None)
    c = subprocess.run([sys.executable, __file__, "--leg", what, str(runs), str(warmup)], capture_output=True, text=True, env=env,
                       timeout=900)
    if c.returncode != 0:
        sys.exit(f"{what} {tree}: exit status {c.returncode}\n{c.stderr[-3000:]}")
    return json.loads(c.stdout.strip().splitlines()[-1])


def main():
    old, new = sys.argv[1], sys.argv[2]
    runs, warmup = 5, 2
    print(f"{N} robots x {STEPS} steps, doggo 2x64, persistent tile; synchronous calls; ms")
    agg = {old: {"evaluate": [], "follow": []}, new: {"evaluate": [], "follow": []}}
    for lib in (old, new, old, new):
        r = child("existing", lib, runs, warmup)
        for k in r:
            agg[lib][k] += r[k]
    print("(a) existing calls, two alternating children per library, 5 runs after 2 warm-up each: min / median / max")
    for k in ("evaluate", "follow"):
        for tag, lib in (("parent", old), ("branch", new)):
            t = 1e3 * np.array(agg[lib][k])
            print(f"  {k:<9} {tag}  {t.min():8.2f} {np.median(t):8.2f} {t.max():8.2f}")
    h = child("hazards", new, runs, warmup)
    print("(b) hazard calls (branch): median ms, ratio to the same call without hazards in the same process, violation rate")
    base = {k: float(np.median(h[k])) for k in ("evaluate", "follow")}
    print(f"  without hazards: evaluate {1e3 * base['evaluate']:.2f}, follow {1e3 * base['follow']:.2f}")
    for M in (0, 16, 256, 1024):
        for S in (1, N):
            for k in ("evaluate", "follow"):
                m = float(np.median(h[f"{k} M={M} S={S}"]))
                print(f"  {k:<9} M={M:<5} S={S:<5} {1e3 * m:9.2f} ms  x{m / base[k]:.2f}  violation rate {h[f'viol M={M} S={S}'][0]:.3f}")


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--leg":
        fn = leg_existing if sys.argv[2] == "existing" else leg_hazards
        print(json.dumps(fn(int(sys.argv[3]), int(sys.argv[4]))))
    else:
        main()
