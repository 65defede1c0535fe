#!/usr/bin/env python3
"""Wall time of one device evaluation / waypoint-following call of a doggo 2x256 policy on k_goal256_tile
(PPOEngine.set_eval_tile256(True)) against the per-step path of the same build, on ONE engine in ONE process, the two
alternating call by call; beside it the 2x64 tile (k_goal64_tile) at the same shape, the yardstick for what one launch reaches.
The calls are synchronous (they return after the results are copied out), so host wall time brackets the whole launch
sequence.  Median (min .. max) of --runs calls per leg after --warmup; the per-step leg gets --perstep-runs calls (it is ~1 s each
at 4096 x 1000)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def engine(H):
    from mobrob_amd.engine import PPOEngine
    from oracle import ppo_oracle as O
    e = PPOEngine(obs_dim=58, act_dim=12, n_envs=16, n_steps=16, batch_size=64, n_epochs=1, pi=(H, H), vf=(H, H), seed=1)
    e.set_params(O.init_params(58, 12, (H, H), (H, H), seed=0))
    return e


def alternate(legs, runs, warmup):
    """legs: [(name, call, runs or None)] -> {name: (times, last result)}; the legs take turns call by call"""
    out = {name: ([], None) for name, _, _ in legs}
    for i in range(warmup + runs):
        for name, call, own in legs:
            if i >= warmup + (runs if own is None else own):
                continue
            t0 = time.perf_counter()
            r = call()
            dt = time.perf_counter() - t0
            ts, _ = out[name]
            if i >= warmup:
                ts.append(dt)
            out[name] = (ts, r)
    return out


def report(title, out, steps):
    print(title)
    for name, (ts, r) in out.items():
        ts = np.asarray(ts)
        print(f"  {name:<44} {1e3 * np.median(ts):9.2f} ms  ({1e3 * ts.min():.2f} .. {1e3 * ts.max():.2f}, {len(ts)} calls)"
              f"  {1e6 * np.median(ts) / steps:8.2f} us/step  persistent={r['persistent']}  mean reward {r['reward_sum'].mean():.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, nargs="+", default=[4096, 1024, 256])
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--perstep-runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    from mobrob_amd.envs.vec_env import DeviceGoalVecEnv
    os.environ.pop("MOBROB_EVAL_PERSISTENT", None)
    os.environ.pop("MOBROB_EVAL_TILE256", None)
    e256, e64 = engine(256), engine(64)

    def on(flag, call):
        def run():
            e256.set_eval_tile256(flag)
            return call()
        return run
    for n in a.robots:
        env = DeviceGoalVecEnv.for_robot("doggo", n, time_limit=0)
        ev = lambda e: (lambda: env.evaluate(e, n_robots=n, max_steps=a.steps, episodes=0, seed=1))   # noqa: E731
        out = alternate([("2x256 tile (k_goal256_tile<EvalTask>)", on(True, ev(e256)), None),
                         ("2x256 per-step (x3 forward + step kernel)", on(False, ev(e256)), a.perstep_runs),
                         ("2x64 tile (k_goal64_tile<64, EvalTask>)", ev(e64), None)], a.runs, a.warmup)
        report(f"evaluate: {n} robots x {a.steps} steps, control.py protocol, median of {a.runs} after {a.warmup} warm-up", out, a.steps)
        t, p = (np.median(out[k][0]) for k in list(out)[:2])
        print(f"  tile against per-step: x{p / t:.1f}")
    n = a.robots[0]
    env = DeviceGoalVecEnv.for_robot("doggo", n, time_limit=0)
    rng = np.random.default_rng(0)
    start = rng.uniform(-1.5, 1.5, (n, 2)).astype(np.float32)
    wp = rng.uniform(-2.0, 2.0, (n, 4, 2)).astype(np.float32)
    fo = lambda e: (lambda: env.follow(e, start, wp, max_steps=a.steps, seed=1))   # noqa: E731
    out = alternate([("2x256 tile (k_goal256_tile<FollowTask>)", on(True, fo(e256)), None),
                     ("2x256 per-step", on(False, fo(e256)), a.perstep_runs),
                     ("2x64 tile (k_goal64_tile<64, FollowTask>)", fo(e64), None)], a.runs, a.warmup)
    report(f"follow_waypoints: {n} robots x {a.steps} steps, 4 waypoints", out, a.steps)
    t, p = (np.median(out[k][0]) for k in list(out)[:2])
    print(f"  tile against per-step: x{p / t:.1f}")


if __name__ == "__main__":
    main()
