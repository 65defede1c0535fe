#!/usr/bin/env python3
"""Wall time of one device waypoint-following call (mobrob_ppo_follow_waypoints) of 4096 robots x 1000 steps at doggo 2x64:
the persistent kernel (k_goal64_tile<FollowTask>), the per-step path (MOBROB_EVAL_PERSISTENT=0) and, for comparison at the same shape,
one evaluation (k_goal64_tile<EvalTask>, control.py protocol).  The host loop (mobrob_amd.waypoints, one predict per robot and step) runs
for --host-robots robots and is extrapolated to 4096 (labelled as such).  Every robot follows a 4-corner square far enough from
its start that no robot finishes early with this untrained actor, so every call runs the full 1000 steps.  The calls are
synchronous (they return after the results are copied out); median of --runs after --warmup.
--only persistent: one persistent follow call (a rocprofv3 kernel trace)."""
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


def timed(fn, runs, warmup):
    ts = []
    for i in range(warmup + runs):
        t0 = time.perf_counter()
        r = fn()
        if i >= warmup:
            ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-robots", type=int, default=2)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    from mobrob_amd.envs.vec_env import DeviceGoalVecEnv
    from mobrob_amd.waypoints import follow_waypoints
    env = DeviceGoalVecEnv.for_robot("doggo", a.robots, time_limit=0)
    square = 2.5 * np.array([[1.0, 1.0], [1.0, -1.0], [-1.0, -1.0], [-1.0, 1.0]], np.float32)
    start = np.random.default_rng(0).uniform(-0.5, 0.5, (a.robots, 2)).astype(np.float32)
    e64 = engine(64)

    def follow():
        return env.follow(e64, start, square, max_steps=a.steps, seed=1)
    if a.only == "persistent":
        r = follow()
        print(f"persistent={r['persistent']} mean reward {r['reward_sum'].mean():.4f} mean reached {r['reached'].mean():.3f}")
        return
    rows = []
    os.environ.pop("MOBROB_EVAL_PERSISTENT", None)
    tp, rp = timed(follow, a.runs, a.warmup)
    rows.append(("follow, persistent (k_goal64_tile<FollowTask>)", tp, rp))
    te, re_ = timed(lambda: env.evaluate(e64, n_robots=a.robots, max_steps=a.steps, episodes=0, seed=1), a.runs, a.warmup)
    rows.append(("evaluate, persistent (k_goal64_tile<EvalTask>), same shape", te, re_))
    os.environ["MOBROB_EVAL_PERSISTENT"] = "0"
    ts, rs = timed(follow, max(1, a.runs // 2), 1)
    rows.append(("follow, per-step (fused forward + k_goal_task_step)", ts, rs))
    os.environ.pop("MOBROB_EVAL_PERSISTENT", None)

    class _Predict:   # the same engine behind PPO.predict's call shape
        def predict(self, obs, deterministic=True):
            return e64.predict(np.asarray(obs, np.float32), deterministic=deterministic), None
    hn = a.host_robots
    t0 = time.perf_counter()
    rh = follow_waypoints(_Predict(), "doggo", start[:hn], square, max_steps=a.steps, seed=1)
    th = time.perf_counter() - t0
    print(f"{a.robots} robots x {a.steps} steps, doggo 2x64 (obs 58, act 12), square path of 4 waypoints, "
          f"median of {a.runs} after {a.warmup} warm-up (per-step path: median of {max(1, a.runs // 2)} after 1)")
    for name, t, r in rows:
        print(f"  {name:<56} {1e3 * t:9.2f} ms  {1e6 * t / a.steps:8.2f} us/step  mean reward {r['reward_sum'].mean():.4f}"
              f"  persistent={r['persistent']}")
    print(f"  {'host loop, ' + str(hn) + ' robots measured (' + str(int(rh['steps'].sum())) + ' predict calls)':<56} {1e3 * th:9.2f} ms")
    print(f"  {'host loop, EXTRAPOLATED to ' + str(a.robots) + ' robots (x' + str(a.robots // hn) + ')':<56} "
          f"{1e3 * th * a.robots / hn:9.0f} ms")
    print(f"  follow persistent / evaluate persistent: {tp / te:.2f}x;  per-step / persistent: {ts / tp:.1f}x")


if __name__ == "__main__":
    main()
