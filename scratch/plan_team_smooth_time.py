"""Times one mobrob_ppo_plan_grid_team_smooth call beside mobrob_ppo_plan_grid_team of the same run on the same scene, the shape of
scratch/plan_team_time.py: 4096 robots, the enclosure plus 16 boxes, G in {64, 128}, T in {16, 64}, teams of 2 and 16, max_leg 8,
margin 0 and 1.  Host clock around a call that ends in a stream synchronise, `warm` warm-up calls, median of `runs`.  Both calls are
timed without the host's clearance check (clearance=False), so both sides are the device call and its copies.  k_plan_team and its
host path are the previous build's, unchanged.  Prints one line per case; record them in profiles/r22/plan_team_smooth.txt.
    python scratch/plan_team_smooth_time.py [runs [warm [G,G.. [T,T..]]]]"""
import statistics
import sys
import time

import numpy as np

from mobrob_amd.engine import PPOEngine
from mobrob_amd.envs.goal_rules import GridSpec, Teams, Walls


def median_ms(call, runs, warm):
    for _ in range(warm):
        call()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    runs, warm = (int(sys.argv[1]) if len(sys.argv) > 1 else 20), (int(sys.argv[2]) if len(sys.argv) > 2 else 3)
    grids = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [64, 128]
    layers = [int(v) for v in sys.argv[4].split(",")] if len(sys.argv) > 4 else [16, 64]
    rng = np.random.default_rng(0)
    n = 4096
    boxes = np.concatenate([Walls.enclosure(3.6, 0.2), np.column_stack([rng.uniform(-1.3, 1.3, (16, 2)), rng.uniform(0.05, 0.2, (16, 2))])])
    walls = Walls(boxes, radius=0.05)
    start = rng.uniform(-1.5, 1.5, (n, 2)).astype(np.float32)
    goals16 = rng.uniform(-1.5, 1.5, (16, 2)).astype(np.float32)
    goal = goals16[np.arange(n) % 16]
    e = PPOEngine(obs_dim=8, act_dim=2, n_envs=16, n_steps=8, batch_size=64, n_epochs=1, pi=(64, 64), vf=(64, 64), seed=0)
    for G in grids:
        spec = GridSpec(2.0, G)
        for T in layers:
            for size in (2, 16):
                kw = dict(teams=Teams(size, 0.1), reserve=1, start=start, goal=goal, layer_steps=10, layers=T, max_waypoints=32, clearance=False)
                plain = median_ms(lambda: e.plan_grid_team(spec, walls, None, **kw), runs, warm)
                for margin in (0, 1):
                    smooth = median_ms(lambda: e.plan_smooth_team(spec, walls, None, margin=margin, max_leg=8, **kw), runs, warm)
                    print(f"G = {G:3d}, T = {T:2d}, teams of {size:2d}, margin {margin}: team plan {plain:.2f} ms, smoothed team plan {smooth:.2f} ms "
                          f"({smooth / plain:.2f} x)", flush=True)
    e.close()


if __name__ == "__main__":
    main()
