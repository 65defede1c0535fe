#!/usr/bin/env python3
"""Wall time of one clearance-aware grid-planner call beside plan_grid of the SAME run (profiles/r26/plan_clear.txt).

  python scratch/plan_clear_time.py [OUT.json]
scratch/plan_time.py's scene and robots (4096 robots, the enclosure plus 16 boxes, extent 3), G = 64 and 128, 16 shared goals and
4096 distinct goals.  The two calls ALTERNATE, one timed call of each a round, median of 20 rounds after 3 warm-up rounds, host clock
around the call (which ends in a stream synchronise): a full call (occupancy, [surcharges,] fields, paths), the replanning round on
the resident fields (the two families stay resident side by side), and the smoothing call at margin 1.  Beside them the sweep counts
of the two relaxations.  In the 16-goal cases the first 256 robots are compared with the NumPy rule."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
N, K, CLEARANCE = 4096, 32, (2, 8)


def alternate_ms(fa, fb, runs, warmup):
    """the medians of fa and fb, timed in turn"""
    ta, tb = [], []
    for r in range(warmup + runs):
        for fn, t in ((fa, ta), (fb, tb)):
            t0 = time.perf_counter()
            fn()
            if r >= warmup:
                t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ta)), float(np.median(tb))


def main(out_path=None, runs=20, warmup=3):
    from plan_time import free_points, scene
    from mobrob_amd.engine import PPOEngine
    from mobrob_amd.envs import goal_rules as R
    e = PPOEngine(obs_dim=14, act_dim=2, n_envs=16, n_steps=16, batch_size=64, n_epochs=1, pi=(64, 64), vf=(64, 64), seed=1)
    rng = np.random.default_rng(11)
    walls = scene(rng)
    start, goals16, distinct = free_points(rng, walls, N), free_points(rng, walls, 16), free_points(rng, walls, N)
    moved = start[::-1].copy()
    res = {}
    for G in (64, 128):
        spec = R.GridSpec(3.0, G)
        for name, goal in (("16 shared goals", goals16[np.arange(N) % 16]), ("4096 distinct goals", distinct)):
            kw = dict(start=start, goal=goal, max_waypoints=K)
            plain = e.plan_grid(spec, walls, None, **kw)
            clear = e.plan_grid_clear(spec, walls, None, clearance=CLEARANCE, **kw)
            row = {"fields": int(len(plain["field_goal_cell"])), "clearance": list(CLEARANCE),
                   "sweeps_plain": [int(plain["sweeps"].min()), float(plain["sweeps"].mean()), int(plain["sweeps"].max())],
                   "sweeps_clear": [int(clear["sweeps"].min()), float(clear["sweeps"].mean()), int(clear["sweeps"].max())],
                   "status_counts_clear": np.bincount(clear["status"], minlength=4).tolist()}
            a, b = alternate_ms(lambda: e.plan_grid(spec, walls, None, **kw),
                                lambda: e.plan_grid_clear(spec, walls, None, clearance=CLEARANCE, **kw), runs, warmup)
            row["full_ms"] = {"plan_grid": a, "plan_grid_clear": b, "ratio": b / a}
            plain = e.plan_grid(spec, walls, None, **kw)
            clear = e.plan_grid_clear(spec, walls, None, clearance=CLEARANCE, **kw)
            a, b = alternate_ms(lambda: e.plan_grid(spec, walls, None, start=moved, goal=goal, max_waypoints=K, reuse=plain),
                                lambda: e.plan_grid_clear(spec, walls, None, clearance=CLEARANCE, start=moved, goal=goal, max_waypoints=K,
                                                          reuse=clear), runs, warmup)
            row["paths_only_ms"] = {"plan_grid": a, "plan_grid_clear": b, "ratio": b / a}
            a, b = alternate_ms(lambda: e.plan_smooth(spec, reuse=plain, start=moved, goal=goal, max_waypoints=K, margin=1),
                                lambda: e.plan_smooth_clear(spec, reuse=clear, start=moved, goal=goal, max_waypoints=K, margin=1), runs, warmup)
            row["smooth_margin1_ms"] = {"plan_smooth": a, "plan_smooth_clear": b, "ratio": b / a}
            sp, sc = (e.plan_smooth(spec, reuse=plain, start=start, goal=goal, max_waypoints=K, margin=1),
                      e.plan_smooth_clear(spec, reuse=clear, start=start, goal=goal, max_waypoints=K, margin=1))
            ok = (sp["status"] == 0) & (sc["status"] == 0)
            row["margin1_waypoints_mean"] = {"plain": float(sp["count"][ok].mean()), "clear": float(sc["count"][ok].mean())}
            row["moves_mean"] = {"plain": float(sp["moves"][ok].mean()), "clear": float(sc["moves"][ok].mean())}
            row["clearance_min_mean"] = float(sc["clearance_min"][ok].mean())
            if name.startswith("16"):
                ref = R.grid_plan(spec, walls, None, start[:256], goal[:256], K, clearance=CLEARANCE)   # the rule on the first 256 robots
                got = e.plan_grid_clear(spec, walls, None, clearance=CLEARANCE, **kw)
                row["equal_to_rule_256"] = bool(all(np.array_equal(got[k][:256], ref[k]) for k in ("waypoints", "count", "status", "cost",
                                                                                                 "clearance_min")))
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
