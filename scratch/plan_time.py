#!/usr/bin/env python3
"""Wall time of one grid-planner call at 4096 robots (profiles/r17/plan.txt).

  python scratch/plan_time.py [OUT.json]
Scene: the enclosure plus 16 boxes, extent 3.  For G = 64 and 128: a full call (occupancy, fields, paths; host clock around the
call, which ends in a stream synchronise) with 16 goals shared among the robots and with 4096 distinct goals; the replanning round
on the resident fields (the path kernel alone) beside it; the sweep counts of the fields; and the NumPy rule on the same machine,
timed on the 16 shared fields (occupancy + 16 grid_field + 4096 grid_path) and scaled by fields for the distinct goals.  Every
device result is compared with the rule where the rule was run (the 16-goal cases)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, K = 4096, 32


def scene(rng):
    from mobrob_amd.envs.goal_rules import Walls
    boxes = np.concatenate([rng.uniform(-1.1, 1.1, (16, 2)), rng.uniform(0.01, 0.08, (16, 2))], axis=-1)
    return Walls(np.concatenate([Walls.enclosure(), boxes]), radius=0.05)


def free_points(rng, walls, n):
    """n points inside the enclosure whose cell is free at 64 and at 128 cells (a start or goal in a blocked cell has no plan)"""
    from mobrob_amd.envs import goal_rules as R
    pts = rng.uniform(-1.15, 1.15, (8 * n, 2)).astype(np.float32)
    ok = np.ones(len(pts), bool)
    for G in (64, 128):
        spec = R.GridSpec(3.0, G)
        ix, iy = spec.cell_of(pts)
        ok &= ~R.grid_occupancy(spec, walls)[0][iy, ix]
    return pts[ok][:n]


def median_ms(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def main(out_path=None, runs=20, warmup=3):
    from mobrob_amd.engine import PPOEngine
    from mobrob_amd.envs import goal_rules as R
    e = PPOEngine(obs_dim=14, act_dim=2, n_envs=16, n_steps=16, batch_size=64, n_epochs=1, pi=(64, 64), vf=(64, 64), seed=1)
    rng = np.random.default_rng(11)
    walls = scene(rng)
    start, goals16, distinct = free_points(rng, walls, N), free_points(rng, walls, 16), free_points(rng, walls, N)
    assert len(start) == N and len(goals16) == 16 and len(distinct) == N
    res = {}
    for G in (64, 128):
        spec = R.GridSpec(3.0, G)
        for name, goal in (("16 shared goals", goals16[np.arange(N) % 16]), ("4096 distinct goals", distinct)):
            full = e.plan_grid(spec, walls, None, start=start, goal=goal, max_waypoints=K)
            row = {"fields": int(len(full["field_goal_cell"])), "sweeps_min": int(full["sweeps"].min()), "sweeps_max": int(full["sweeps"].max()),
                   "sweeps_mean": float(full["sweeps"].mean()), "status_counts": np.bincount(full["status"], minlength=4).tolist()}
            row["full_ms"] = median_ms(lambda: e.plan_grid(spec, walls, None, start=start, goal=goal, max_waypoints=K), runs, warmup)
            kept = e.plan_grid(spec, walls, None, start=start, goal=goal, max_waypoints=K)
            moved = start[::-1].copy()
            row["paths_only_ms"] = median_ms(lambda: e.plan_grid(spec, walls, None, start=moved, goal=goal, max_waypoints=K, reuse=kept), runs, warmup)
            if name.startswith("16"):
                t0 = time.perf_counter()
                ref = R.grid_plan(spec, walls, None, start, goal, K)
                row["numpy_rule_ms"] = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                occ = R.grid_occupancy(spec, walls)
                for f in range(len(ref["field_goal_cell"])):
                    R.grid_field(occ[0], ref["field_goal_cell"][f])
                row["numpy_fields_ms"] = (time.perf_counter() - t0) * 1e3
                row["equal_to_rule"] = bool(all(np.array_equal(full[k], ref[k]) for k in ("waypoints", "count", "status", "cost")))
                res[f"G{G} numpy per field ms"] = row["numpy_fields_ms"] / 16
                res[f"G{G} numpy per path ms"] = (row["numpy_rule_ms"] - row["numpy_fields_ms"]) / N
            else:   # scaled from the 16-field run: fields x per-field time + robots x per-path time
                row["numpy_rule_ms_scaled"] = row["fields"] * res[f"G{G} numpy per field ms"] + N * res[f"G{G} numpy per path ms"]
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
