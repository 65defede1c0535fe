"""Times one mobrob_ppo_spec_plan call beside a mobrob_ppo_plan_grid call of the same run that computes the same number of fields (the
yardstick: the fields should dominate, the station, tour and path kernels be a small addition), and beside the NumPy rule
(goal_rules.spec_plan, one run): 4096 robots, the enclosure plus 16 boxes, two keep-out boxes as avoid clauses, every start in a free cell, G in {64, 128}, M in
{4, 8} stations (one scene, no goal: M fields), every second station with a window or a dwell.  Host clock around a call that ends
in a stream synchronise, `warm` warm-up calls, median of `runs`.  Prints one line per case; record them in
profiles/r34/plan_spec.txt.
    python scratch/plan_spec_time.py [runs [warm [G,G..]]]"""
import sys
import time

import numpy as np

from mobrob_amd.engine import PPOEngine
from mobrob_amd.envs import goal_rules as R
from scratch.plan_team_rounds_time import median_ms


def main():
    runs, warm = (int(sys.argv[1]) if len(sys.argv) > 1 else 10), (int(sys.argv[2]) if len(sys.argv) > 2 else 2)
    grids = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [64, 128]
    rng = np.random.default_rng(0)
    n = 4096
    boxes = np.concatenate([R.Walls.enclosure(3.6, 0.2), np.column_stack([rng.uniform(-1.3, 1.3, (16, 2)), rng.uniform(0.05, 0.2, (16, 2))])])
    walls = R.Walls(boxes, radius=0.05)
    keep_out = [[0.6, -0.4, 0.2, 0.1], [-0.7, 0.5, 0.1, 0.2]]
    cand = rng.uniform(-1.5, 1.5, (4 * n, 2)).astype(np.float32)       # starts in cells that are free on every grid timed: every robot walks
    free = np.ones(len(cand), bool)
    for G in grids:
        occ = R.spec_plan_occupancy(R.GridSpec(2.0, G), walls, None, R.Regions(keep_out, [0, 0]), [(0, 2)])[0]
        sx, sy = R.GridSpec(2.0, G).cell_of(cand)
        free &= ~occ[sy, sx]
    start = np.ascontiguousarray(cand[free][:n])
    assert len(start) == n
    e = PPOEngine(obs_dim=8, act_dim=2, n_envs=16, n_steps=8, batch_size=64, n_epochs=1, pi=(64, 64), vf=(64, 64), seed=0)
    for G in grids:
        grid = R.GridSpec(2.0, G)
        for M in (4, 8):
            centres = rng.uniform(-1.4, 1.4, (M, 2))
            rows = np.concatenate([np.column_stack([centres, np.full(M, 0.25), np.zeros(M)]), keep_out])
            reg = R.Regions(rows, [1] * M + [0, 0])
            clauses = [R.Spec.eventually(R.inside(j)) if j % 2 == 0 else (R.Spec.stay(R.inside(j), 5, 0, None) if j % 4 == 1 else
                                                                         R.Spec.eventually(R.inside(j), 40, None)) for j in range(M)]
            spec = R.Spec(reg, clauses + [R.Spec.always(R.outside(M, M + 2))])
            kw = dict(spec=spec, start=start, pace=2, max_waypoints=64)
            ms = median_ms(lambda: e.plan_spec(grid, walls, None, **kw), runs, warm)
            out = e.plan_spec(grid, walls, None, **kw)
            goal = centres[np.arange(n) % M].astype(np.float32)             # as many distinct goal cells as the stations have fields
            ref = median_ms(lambda: e.plan_grid(grid, walls, None, start=start, goal=goal, max_waypoints=64), runs, warm)
            n_fields = len(e.plan_grid(grid, walls, None, start=start, goal=goal, max_waypoints=64)["field_goal_cell"])
            t0 = time.perf_counter()
            rule = R.spec_plan(grid, walls, None, spec, start, None, 64, 2)
            numpy_s = time.perf_counter() - t0
            same = all(np.array_equal(out[k], rule[k]) for k in ("waypoints", "count", "status", "cost", "tour_order", "release"))
            print(f"G = {G:3d}, M = {M}: plan_spec {ms:.2f} ms ({M} fields), plan_grid {ref:.2f} ms ({n_fields} fields): {ms / ref:.2f} x; "
                  f"NumPy rule {numpy_s:.1f} s; planned {int((out['status'] == 0).sum())}, none {int((out['status'] == 1).sum())}, truncated "
                  f"{int((out['status'] == 2).sum())}, unconverged {int((out['status'] == 3).sum())}; holds {int((out['release'] != 0).sum())}; "
                  f"equal to the rule: {same}", flush=True)
    e.close()


if __name__ == "__main__":
    main()
