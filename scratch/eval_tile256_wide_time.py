#!/usr/bin/env python3
"""Wall time of one waypoint-following call WITH 16 hazards of a doggo 2x256 policy, by the method of eval_tile256_time.py (one
process, legs alternating call by call, median (min .. max) of --runs after --warmup, --perstep-runs calls for per-step legs):
  (a) the wide tile        k_goal256_tile<HazardTask<FollowTask>>         set_eval_tile256(True) + set_eval_tile256_wide(True)
  (b) the per-step path    of the same build with the wide switch off     (what every such call ran before: the bar)
  (c) the unwrapped tile   k_goal256_tile<FollowTask>                     the same call without hazards
  (d) the 2x64 tile        k_goal64_tile<64, HazardTask<FollowTask>>      and (d0) k_goal64_tile<64, FollowTask>
and the ratios (a)/(c) beside (d)/(d0): whether the wide phase costs more at four waves than at one.  (a) must beat (b) by more
than the spread of either leg at every robot count for the task to stay in task_tile256_wide.  Walls, solid walls and teams are
not served by the 256-wide tile and are not timed here."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scratch.eval_tile256_time import alternate, engine, report   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, nargs="+", default=[4096, 1024, 256])
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--hazards", type=int, default=16)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--perstep-runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    from mobrob_amd.envs.goal_rules import Hazards
    from mobrob_amd.envs.vec_env import DeviceGoalVecEnv
    for k in ("MOBROB_EVAL_PERSISTENT", "MOBROB_EVAL_TILE256", "MOBROB_EVAL_TILE256_WIDE"):
        os.environ.pop(k, None)
    e256, e64 = engine(256), engine(64)
    e256.set_eval_tile256(True)
    hz = Hazards(np.random.default_rng(2).uniform(-2.0, 2.0, (a.hazards, 2)), 0.3, cost=1.0, indicator=False)

    def wide(flag, call):
        def run():
            e256.set_eval_tile256_wide(flag)
            return call()
        return run
    for n in a.robots:
        env = DeviceGoalVecEnv.for_robot("doggo", n, time_limit=0)
        rng = np.random.default_rng(0)
        start = rng.uniform(-1.5, 1.5, (n, 2)).astype(np.float32)
        wp = rng.uniform(-2.0, 2.0, (n, 4, 2)).astype(np.float32)
        fo = lambda e, h: (lambda: env.follow(e, start, wp, max_steps=a.steps, seed=1, hazards=h))   # noqa: E731
        out = alternate([("(a) 2x256 wide tile, hazards", wide(True, fo(e256, hz)), None),
                         ("(b) 2x256 per-step, hazards", wide(False, fo(e256, hz)), a.perstep_runs),
                         ("(c) 2x256 tile, no hazards", fo(e256, None), None),
                         ("(d) 2x64 tile, hazards", fo(e64, hz), None),
                         ("(d0) 2x64 tile, no hazards", fo(e64, None), None)], a.runs, a.warmup)
        report(f"follow_waypoints + {a.hazards} hazards: {n} robots x {a.steps} steps, 4 waypoints, median of {a.runs} after {a.warmup} warm-up",
               out, a.steps)
        m = {k[:4].strip("() "): np.median(v[0]) for k, v in out.items()}
        sp = {k[:4].strip("() "): (max(v[0]) - min(v[0])) for k, v in out.items()}
        print(f"  (b)/(a) x{m['b'] / m['a']:.1f}  (b)-(a) {1e3 * (m['b'] - m['a']):.2f} ms against spreads {1e3 * sp['a']:.2f} / {1e3 * sp['b']:.2f} ms"
              f"   (a)/(c) x{m['a'] / m['c']:.2f}   (d)/(d0) x{m['d'] / m['d0']:.2f}")


if __name__ == "__main__":
    main()
