#!/usr/bin/env python3
"""Wall time of a smoothed replanning round at 4096 robots (profiles/r18/plan_smooth.txt), under the conditions of
scratch/plan_time.py (its scene, starts and goals): for G = 64 and 128, with 16 shared goals and with 4096 distinct goals,
  * one k_plan_path round on resident fields (plan_grid with reuse=), as profiles/r17/plan.txt timed it,
  * one smoothed round on the same fields (plan_smooth, margin 0 and margin 1),
  * the first-call totals: plan_grid alone, and plan_grid followed by plan_smooth (what a smoothed first plan costs),
host clock around the calls, each of which ends in a stream synchronise; median [min .. max] of 20 after 3 warm-up calls.  The
16-goal device results are compared with the rule.

  python scratch/plan_smooth_time.py [OUT.json]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from plan_time import K, N, free_points, median_ms, scene   # noqa: E402


def main(out_path=None, runs=20, warmup=3):
    from mobrob_amd.engine import PPOEngine
    from mobrob_amd.envs import goal_rules as R
    e = PPOEngine(obs_dim=14, act_dim=2, n_envs=16, n_steps=16, batch_size=64, n_epochs=1, pi=(64, 64), vf=(64, 64), seed=1)
    rng = np.random.default_rng(11)
    walls = scene(rng)
    start, goals16, distinct = free_points(rng, walls, N), free_points(rng, walls, 16), free_points(rng, walls, N)
    res = {}
    for G in (64, 128):
        spec = R.GridSpec(3.0, G)
        for name, goal in (("16 shared goals", goals16[np.arange(N) % 16]), ("4096 distinct goals", distinct)):
            moved = start[::-1].copy()
            kept = e.plan_grid(spec, walls, None, start=start, goal=goal, max_waypoints=K, want_occupancy=True, want_fields=True)
            row = {"fields": int(len(kept["field_goal_cell"]))}
            row["paths_only_ms"] = median_ms(lambda: e.plan_grid(spec, walls, None, start=moved, goal=goal, max_waypoints=K, reuse=kept), runs, warmup)
            raw = e.plan_grid(spec, walls, None, start=moved, goal=goal, max_waypoints=K, reuse=kept)
            row["waypoints_unsmoothed"] = int(raw["count"].sum())
            for m in (0, 1):
                sm = e.plan_smooth(spec, reuse=kept, start=moved, goal=goal, max_waypoints=K, margin=m)
                row[f"smooth_m{m}_ms"] = median_ms(lambda: e.plan_smooth(spec, reuse=kept, start=moved, goal=goal, max_waypoints=K, margin=m), runs, warmup)
                row[f"waypoints_m{m}"] = int(sm["count"].sum())
                row[f"status_m{m}"] = np.bincount(sm["status"], minlength=4).tolist()
                row["moves_mean_max"] = [float(sm["moves"].mean()), int(sm["moves"].max())]
                if name.startswith("16"):
                    ref = R.grid_plan(spec, walls, None, moved, goal, K, kept["occupancy"], kept["fields"], smooth=True, margin=m)
                    row[f"equal_to_rule_m{m}"] = bool(all(np.array_equal(sm[k], ref[k]) for k in ("waypoints", "count", "status", "cost", "moves")))
            row["first_call_ms"] = median_ms(lambda: e.plan_grid(spec, walls, None, start=start, goal=goal, max_waypoints=K), runs, warmup)

            def first_smoothed():
                full = e.plan_grid(spec, walls, None, start=start, goal=goal, max_waypoints=K)
                e.plan_smooth(spec, reuse=full, start=start, goal=goal, max_waypoints=K, margin=1)
            row["first_call_smoothed_m1_ms"] = median_ms(first_smoothed, runs, warmup)
            res[f"G{G} {name}"] = row
            print(f"G{G} {name}: {json.dumps(row)}", flush=True)
    e.close()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
