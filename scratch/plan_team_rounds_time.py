"""Times one mobrob_ppo_plan_grid_team_rounds call at retries 0, 2 and 8 beside mobrob_ppo_plan_grid_team of the same run on the same
scene, the shape of scratch/plan_team_time.py: 4096 robots, the enclosure plus 16 boxes, G = 64, T in {16, 64}, teams of 2 and 16.
Host clock around a call that ends in a stream synchronise, `warm` warm-up calls, median of `runs`.  All calls are timed without the
host's clearance check (clearance=False), so every side is the device call and its copies.  Beside the times: the parked members
(UNREACHABLE or UNCONVERGED) summed over the scene's teams, in index order (team_parked_first) and in the result (team_parked), and
the rounds planned.  Prints one line per case; record them in profiles/r23/plan_team_rounds.txt.
    python scratch/plan_team_rounds_time.py [runs [warm [G,G.. [T,T..]]]]"""
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
    grids = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [64]
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
                for retries in (0, 2, 8):
                    ms = median_ms(lambda: e.plan_grid_team_rounds(spec, walls, None, retries=retries, **kw), runs, warm)
                    out = e.plan_grid_team_rounds(spec, walls, None, retries=retries, **kw)
                    print(f"G = {G:3d}, T = {T:2d}, teams of {size:2d}, retries {retries}: team plan {plain:.2f} ms, with rounds {ms:.2f} ms "
                          f"({ms / plain:.2f} x); parked {int(out['team_parked_first'].sum())} -> {int(out['team_parked'].sum())} of {n}, "
                          f"rounds planned {int(out['team_rounds'].sum())} over {n // size} teams (at most {int(out['team_rounds'].max())})", flush=True)
    e.close()


if __name__ == "__main__":
    main()
