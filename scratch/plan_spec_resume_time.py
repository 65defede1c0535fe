"""Times mobrob_ppo_spec_replan beside mobrob_ppo_spec_plan of the same run, on the scene of scratch/plan_spec_time.py (4096 robots,
the enclosure plus 16 boxes, two keep-out boxes as avoid clauses, every start in a free cell, one scene, no goal, pace 2, K = 64, G in
{64, 128}, M in {4, 8}): the old entry point, the new one at its defaults (a state in which nothing is done: every station to do,
t0 = 0, partial off -- the same plan through k_plan_tour_resume and k_plan_tour_path_legs), and a resumed call with half the stations
done (the even ones) at step 100 with partial on.  Host clock around a call that ends in a stream synchronise, `warm` warm-up calls,
median of `runs`.  For the kernel times run the same script under a kernel trace, in a run of its own.  Record the lines in
profiles/r35/plan_spec_resume.txt.
    python scratch/plan_spec_resume_time.py [runs [warm [G,G..]]]"""
import sys

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
    cand = rng.uniform(-1.5, 1.5, (4 * n, 2)).astype(np.float32)
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
            fresh = R.spec_start(n, spec)
            half = fresh.copy()
            half.val[:, R.spec_plan_clauses(spec)[::2], 0] = 1.0
            old = median_ms(lambda: e.plan_spec(grid, walls, None, **kw), runs, warm)
            new = median_ms(lambda: e.plan_spec(grid, walls, None, state=fresh, **kw), runs, warm)
            res = median_ms(lambda: e.plan_spec(grid, walls, None, state=half, step0=100, partial=True, **kw), runs, warm)
            a, b = e.plan_spec(grid, walls, None, **kw), e.plan_spec(grid, walls, None, state=fresh, **kw)
            c = e.plan_spec(grid, walls, None, state=half, step0=100, partial=True, **kw)
            same = all(np.array_equal(a[k], b[k]) for k in R.SPEC_PLAN_KEYS + ("tour_len", "dropped"))
            print(f"G = {G:3d}, M = {M}: spec_plan {old:.2f} ms, spec_replan at defaults {new:.2f} ms ({new / old:.2f} x), resumed with "
                  f"{M // 2} of {M} stations left {res:.2f} ms ({res / old:.2f} x); planned {int((b['status'] == 0).sum())}; the two entry "
                  f"points equal: {same}; resumed: planned {int((c['status'] == 0).sum())}, dropped a station {int((c['dropped'] != 0).sum())}",
                  flush=True)
    e.close()


if __name__ == "__main__":
    main()
