"""Times mobrob_ppo_spec_plan_share beside mobrob_ppo_spec_replan of the same robots, alternating, on the scene of
scratch/plan_spec_resume_time.py (4096 robots, the enclosure plus 16 boxes, two keep-out boxes as avoid clauses, every start in a
free cell, one scene, no goal, pace 2, K = 64, G in {64, 128}, M in {4, 8}), teams of 2, 4 and 16, both objectives.  Host clock around
a call that ends in a stream synchronise, `warm` warm-up calls of each, then `runs` alternating pairs, the median of each side.  For
the kernel times run the same script under a kernel trace, in a run of its own.  Record the lines in profiles/r36/plan_spec_share.txt.
    python scratch/plan_spec_share_time.py [runs [warm [G,G.. [M,size,objective]]]]      (the last: one shape only, for a trace)"""
import sys
import time

import numpy as np

from mobrob_amd.engine import PPOEngine
from mobrob_amd.envs import goal_rules as R


def main():
    runs, warm = (int(sys.argv[1]) if len(sys.argv) > 1 else 10), (int(sys.argv[2]) if len(sys.argv) > 2 else 2)
    grids = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [64, 128]
    only = sys.argv[4].split(",") if len(sys.argv) > 4 else None
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
            kw = dict(spec=spec, start=start, pace=2, max_waypoints=64, state=R.spec_start(n, spec))
            for size in (2, 4, 16):
                for objective in ("makespan", "sum"):
                    if only is not None and (M, size, objective) != (int(only[0]), int(only[1]), only[2]):
                        continue
                    sides = (lambda: e.plan_spec(grid, walls, None, **kw), lambda: e.plan_spec(grid, walls, None, share=size, objective=objective, **kw))
                    for _ in range(warm):
                        for f in sides:
                            f()
                    took = ([], [])
                    for _ in range(runs):
                        for f, t in zip(sides, took):
                            t0 = time.perf_counter()
                            f()
                            t.append(1e3 * (time.perf_counter() - t0))
                    old, new = (float(np.median(t)) for t in took)
                    out = sides[1]()
                    print(f"G = {G:3d}, M = {M}, teams of {size:2d}, {objective:8s}: spec_replan {old:.2f} ms, spec_plan_share {new:.2f} ms "
                          f"({new / old:.2f} x); teams with an allotment {int(out['team_feasible'].sum())} of {n // size}, members with stations "
                          f"{int((out['share'] != 0).sum())}, mean makespan {out['team_makespan'][out['team_feasible']].mean():.1f} ticks", flush=True)
    e.close()


if __name__ == "__main__":
    main()
