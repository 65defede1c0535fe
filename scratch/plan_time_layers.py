#!/usr/bin/env python3
"""Wall time of one time-plan call at 4096 robots (profiles/r19/plan_time.txt), under the conditions of
scratch/plan_time.py: the enclosure plus 16 boxes, extent 3, 16 circling hazards, median of 20 runs.

  python scratch/plan_time_layers.py [OUT.json]
For G = 64 and 128, T = 16 and 64, 16 shared and 4096 distinct goals: a time-plan call (layer maps, time fields, walks; host clock
around the call, which ends in a stream synchronise) beside a static plan_grid call on the walls timed in the same run, and the
ratio of the two; a case whose time fields exceed PLAN_TIME_MAX_BYTES is recorded as refused.  The NumPy rule is timed on ONE
field (layer maps + grid_time_field).  With 16 goals the device result is compared with the rule at T = 16."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scratch.plan_time import K, N, free_points, median_ms, scene   # noqa: E402

LAYER_STEPS = 10


def main(out_path=None, runs=20, warmup=3):
    from mobrob_amd.engine import PPOEngine
    from mobrob_amd.envs import goal_rules as R
    e = PPOEngine(obs_dim=14, act_dim=2, n_envs=16, n_steps=16, batch_size=64, n_epochs=1, pi=(64, 64), vf=(64, 64), seed=1)
    rng = np.random.default_rng(11)
    walls = scene(rng)
    start, goals16, distinct = free_points(rng, walls, N), free_points(rng, walls, 16), free_points(rng, walls, N)
    hz = R.MovingHazards.circling(rng.uniform(-0.9, 0.9, (16, 2)), travel=0.3, size=0.1, n_frames=126, dt=0.05, frame_steps=1, loop=True)
    res = {}
    for G in (64, 128):
        spec = R.GridSpec(3.0, G)
        for name, goal in (("16 shared goals", goals16[np.arange(N) % 16]), ("4096 distinct goals", distinct)):
            static = median_ms(lambda: e.plan_grid(spec, walls, None, start=start, goal=goal, max_waypoints=K), runs, warmup)
            for T in (16, 64):
                kw = dict(start=start, goal=goal, step0=0, layer_steps=LAYER_STEPS, layers=T, max_waypoints=K)
                row = {"static_ms": static}
                try:
                    first = e.plan_grid_time(spec, walls, hz, **kw)
                except ValueError as ex:
                    row["refused"] = str(ex)
                else:
                    row.update(fields=int(len(first["field_goal_cell"])), status_counts=np.bincount(first["status"], minlength=4).tolist(),
                               waits=int(first["waits"].sum()), time_ms=median_ms(lambda: e.plan_grid_time(spec, walls, hz, **kw), runs, warmup))
                    row["ratio_to_static"] = row["time_ms"][0] / static[0]
                    if name.startswith("16"):
                        t0 = time.perf_counter()
                        occ = R.grid_occupancy_time(spec, walls, hz, 0, LAYER_STEPS, T)
                        R.grid_time_field(occ[0], first["field_goal_cell"][0])
                        row["numpy_one_field_ms"] = (time.perf_counter() - t0) * 1e3
                        if T == 16:
                            ref = R.grid_plan_time(spec, walls, hz, start, goal, K, 0, LAYER_STEPS, T)
                            row["equal_to_rule"] = bool(all(np.array_equal(first[k], ref[k]) for k in ("waypoints", "count", "status", "cost", "waits", "leave", "arrive")))
                res[f"G{G} T{T} {name}"] = row
                print(f"G{G} T{T} {name}: {json.dumps(row)}", flush=True)
    e.close()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
