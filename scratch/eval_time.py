#!/usr/bin/env python3
"""Wall time of one device evaluation (mobrob_ppo_evaluate_goal_env) of 4096 robots x 1000 steps, control.py protocol:
doggo 2x64 on the persistent kernel and on the per-step path (MOBROB_EVAL_PERSISTENT=0), doggo 2x256 on the per-step path.
The call is synchronous (it returns after the results are copied out), so host wall time brackets the whole launch
sequence; median of --runs after --warmup.  --only persistent: one persistent evaluation (a rocprofv3 kernel trace)."""
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


def timed(e, env, n, steps, runs, warmup):
    ts = []
    for i in range(warmup + runs):
        t0 = time.perf_counter()
        r = env.evaluate(e, n_robots=n, max_steps=steps, episodes=0, seed=1)
        if i >= warmup:
            ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None)
    ap.add_argument("--make-checkpoint", metavar="DATA_DIR", default=None,
                    help="write DATA_DIR/policies/doggo-ppo.zip (reference doggo weights, tests/golden) for examples/control.py and exit")
    a = ap.parse_args()
    if a.make_checkpoint:
        from tests.util import _write_checkpoint
        _write_checkpoint(a.make_checkpoint, "doggo")
        return
    from mobrob_amd.envs.vec_env import DeviceGoalVecEnv
    env = DeviceGoalVecEnv.for_robot("doggo", a.robots, time_limit=0)
    if a.only == "persistent":
        e = engine(64)
        r = env.evaluate(e, n_robots=a.robots, max_steps=a.steps, seed=1)
        print(f"persistent={r['persistent']} mean reward {r['reward_sum'].mean():.4f}")
        return
    rows = []
    e64 = engine(64)
    os.environ.pop("MOBROB_EVAL_PERSISTENT", None)
    tp, rp = timed(e64, env, a.robots, a.steps, a.runs, a.warmup)
    rows.append(("doggo 2x64 persistent (k_goal64_tile<EvalTask>)", tp, rp))
    os.environ["MOBROB_EVAL_PERSISTENT"] = "0"
    ts, rs = timed(e64, env, a.robots, a.steps, a.runs, a.warmup)
    rows.append(("doggo 2x64 per-step (fused forward + k_goal_task_step)", ts, rs))
    e256 = engine(256)
    t2, r2 = timed(e256, env, a.robots, a.steps, a.runs, a.warmup)
    rows.append(("doggo 2x256 per-step (x3 forward + k_goal_task_step)", t2, r2))
    os.environ.pop("MOBROB_EVAL_PERSISTENT", None)
    print(f"{a.robots} robots x {a.steps} steps, control.py protocol (no time limit, reset on goal), median of {a.runs} after {a.warmup} warm-up")
    for name, t, r in rows:
        print(f"  {name:<58} {1e3 * t:9.2f} ms  {1e6 * t / a.steps:8.2f} us/step  mean reward {r['reward_sum'].mean():.4f}"
              f"  persistent={r['persistent']}")
    print(f"  speed-up persistent vs per-step at 2x64: {ts / tp:.2f}x")


if __name__ == "__main__":
    main()
