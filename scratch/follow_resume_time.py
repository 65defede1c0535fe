#!/usr/bin/env python3
"""Wall time of the resumable waypoint-following call (mobrob_ppo_follow_waypoints_resume) at doggo 2x64, 4096 robots x 1000 steps
(the shape of profiles/r7/follow.txt: a square no robot finishes, so every call runs all its steps) -> profiles/r12/follow_resume.txt.

  python scratch/follow_resume_time.py PARENT_TREE   (a source tree of the previous commit with its built mobrob_amd/libmobrob_ppo.so)
(a) existing calls: follow_waypoints and evaluate (persistent tile) on both trees, alternating parent / branch / parent / branch,
    --runs timed calls after --warmup each time: the spread of each library over all its runs.
(b) this tree: the plain call, one resumed call of 1000 steps (also with a budget that never binds, so that its test is live), a
    chain of 20 x 50 steps, and one per-step line for a 256-wide engine.
Calls are synchronous (they return after the results are copied out).  Each leg runs in a child process of its own, importing
the package from its tree."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("FOLLOW_TIME_TREE", ROOT))
N, STEPS, H = 4096, 1000, 50


def engine(width):
    from mobrob_amd.engine import PPOEngine
    from oracle import ppo_oracle as O
    e = PPOEngine(obs_dim=58, act_dim=12, n_envs=16, n_steps=16, batch_size=64, n_epochs=1, pi=(width, width), vf=(width, width), seed=1)
    e.set_params(O.init_params(58, 12, (width, width), (width, width), seed=0))
    return e


def setup():
    from mobrob_amd.envs.vec_env import DeviceGoalVecEnv
    env = DeviceGoalVecEnv.for_robot("doggo", N, time_limit=0)
    square = 2.5 * np.array([[1.0, 1.0], [1.0, -1.0], [-1.0, -1.0], [-1.0, 1.0]], np.float32)
    start = np.random.default_rng(0).uniform(-0.5, 0.5, (N, 2)).astype(np.float32)
    return env, square, start


def times(fn, runs, warmup):
    ts, r = [], None
    for i in range(warmup + runs):
        t0 = time.perf_counter()
        r = fn()
        if i >= warmup:
            ts.append(time.perf_counter() - t0)
    return ts, r


def leg_existing(runs, warmup):
    env, square, start = setup()
    e = engine(64)
    tf, r = times(lambda: env.follow(e, start, square, max_steps=STEPS, seed=1), runs, warmup)
    assert r["persistent"] and np.all(r["steps"] == STEPS)
    te, _ = times(lambda: env.evaluate(e, n_robots=N, max_steps=STEPS, seed=1), runs, warmup)
    return {"follow": tf, "evaluate": te}


def leg_resume(runs, warmup):
    from mobrob_amd.waypoints import FollowState
    env, square, start = setup()
    e = engine(64)
    out = {}
    out["plain"], rp = times(lambda: env.follow(e, start, square, max_steps=STEPS, seed=1), runs, warmup)
    assert rp["persistent"] and np.all(rp["steps"] == STEPS)
    fresh = FollowState(start, square, None, False, 2)
    out["resumed"], r1 = times(lambda: env.follow(e, max_steps=STEPS, seed=1, resume=fresh), runs, warmup)
    assert r1["persistent"] and np.array_equal(r1["reward_sum"], rp["reward_sum"]) and np.array_equal(r1["arrival"], rp["arrival"])
    out["budget"], _ = times(lambda: env.follow(e, max_steps=STEPS, seed=1, resume=fresh, leg_steps=1000000), runs, warmup)

    def chain():
        r, s = None, fresh
        for _ in range(STEPS // H):
            r = env.follow(e, max_steps=H, seed=1, resume=s)
            s = r["state"]
        return r
    out["chain"], rc = times(chain, runs, warmup)
    assert np.array_equal(rc["reward_sum"], r1["reward_sum"]) and np.array_equal(rc["state"].state, r1["state"].state)
    out["plain again"], _ = times(lambda: env.follow(e, start, square, max_steps=STEPS, seed=1), runs, warmup)
    e.close()
    e = engine(256)
    out["per-step resumed"], r2 = times(lambda: env.follow(e, max_steps=100, seed=1, resume=fresh), 3, 1)
    out["per-step plain"], _ = times(lambda: env.follow(e, start, square, max_steps=100, seed=1), 3, 1)
    assert not r2["persistent"]
    e.close()
    return out


def child(what, tree, runs, warmup):
    env = dict(os.environ, FOLLOW_TIME_TREE=os.path.abspath(tree))
    for k in ("MOBROB_EVAL_PERSISTENT", "MOBROB_PPO_LIB"):
        env.pop(k, None)
    c = subprocess.run([sys.executable, __file__, "--leg", what, "--runs", str(runs), "--warmup", str(warmup)], capture_output=True,
                       text=True, env=env, timeout=600)
    if c.returncode != 0:
        sys.exit(f"{what} {tree}: exit status {c.returncode}\n{c.stderr[-3000:]}")
    return json.loads(c.stdout.strip().splitlines()[-1])


def line(label, ts):
    t = 1e3 * np.array(ts)
    print(f"  {label:<58} {t.min():9.3f} {np.median(t):9.3f} {t.max():9.3f}", flush=True)
    return float(np.median(t))


def main(a):
    old, new = a.parent, ROOT
    print(f"{N} robots x {STEPS} steps, doggo 2x64, persistent tile; synchronous calls; ms: min / median / max")
    agg = {old: {"follow": [], "evaluate": []}, new: {"follow": [], "evaluate": []}}
    for tree in (old, new, old, new):
        r = child("existing", tree, a.runs, a.warmup)
        for k in r:
            agg[tree][k] += r[k]
    print(f"(a) existing calls, two alternating children per library, {a.runs} runs after {a.warmup} warm-up each")
    for k in ("follow", "evaluate"):
        for tag, tree in (("parent", old), ("branch", new)):
            line(f"{k:<9} {tag}", agg[tree][k])
    r = child("resume", new, a.runs, a.warmup)
    n = STEPS // H
    print(f"(b) resumable call (branch), one process, {a.runs} runs after {a.warmup} warm-up each")
    tp = line("follow_waypoints, k_goal64_tile<FollowTask>", r["plain"])
    t1 = line("resumed call, 1000 steps, k_goal64_tile<ResumeFollowTask>", r["resumed"])
    tb = line("resumed call, leg_steps = 1000000 (budget test live)", r["budget"])
    tc = line(f"chain of {n} resumed calls x {H} steps", r["chain"])
    line("follow_waypoints again (drift of the process)", r["plain again"])
    print(f"  resumed / plain = {t1 / tp:.3f}; with a budget / plain = {tb / tp:.3f}")
    print(f"  chain / one resumed call = {tc / t1:.3f}; per call of {H} steps {tc / n:.3f} ms, of which steps {t1 / n:.3f} ms and "
          f"per-call overhead {(tc - t1) / n:.3f} ms (actor -> LDS, launch, copies in and out, Python)")
    print("(c) per-step path, one 2x256 engine, 100 steps, 3 runs after 1 warm-up")
    t2 = line("resumed call (k_goal_task_init / _step / _fin)", r["per-step resumed"])
    t3 = line("follow_waypoints", r["per-step plain"])
    print(f"  resumed / plain = {t2 / t3:.3f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("parent", nargs="?")
    ap.add_argument("--leg", choices=("existing", "resume"))
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.leg:
        print(json.dumps((leg_existing if a.leg == "existing" else leg_resume)(a.runs, a.warmup)))
    elif a.parent:
        main(a)
    else:
        ap.error("PARENT_TREE is required")
