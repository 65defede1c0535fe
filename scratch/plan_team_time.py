"""Times one mobrob_ppo_plan_grid_team call beside mobrob_ppo_plan_grid_time of the same run on the same scene: 4096 robots, the
enclosure plus 16 boxes, G in {64, 128}, T in {16, 64}, teams of 2 and 16.  Host clock around a call that ends in a stream
synchronise, 3 warm-up calls, median of 20.  The team call is timed without the host's clearance check (clearance=False), so both
sides are the device call and its copies.  Prints one line per case; record them in profiles/r20/plan_team.txt."""
import statistics
import time

import numpy as np

from mobrob_amd.engine import PPOEngine
from mobrob_amd.envs.goal_rules import GridSpec, MovingHazards, Teams, Walls


def median_ms(call, runs=20, warm=3):
    for _ in range(warm):
        call()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    rng = np.random.default_rng(0)
    n = 4096
    boxes = np.concatenate([Walls.enclosure(3.6, 0.2), np.column_stack([rng.uniform(-1.3, 1.3, (16, 2)), rng.uniform(0.05, 0.2, (16, 2))])])
    walls = Walls(boxes, radius=0.05)
    parked = MovingHazards(np.array([[(1.95, 1.95)]]), size=0.01)          # one frame outside the enclosure: the time plan's static scene
    start = rng.uniform(-1.5, 1.5, (n, 2)).astype(np.float32)
    goals16 = rng.uniform(-1.5, 1.5, (16, 2)).astype(np.float32)
    goal = goals16[np.arange(n) % 16]
    e = PPOEngine(obs_dim=8, act_dim=2, n_envs=16, n_steps=8, batch_size=64, n_epochs=1, pi=(64, 64), vf=(64, 64), seed=0)
    for G in (64, 128):
        spec = GridSpec(2.0, G)
        for T in (16, 64):
            alone = median_ms(lambda: e.plan_grid_time(spec, walls, parked, start=start, goal=goal, layer_steps=10, layers=T, max_waypoints=32))
            for size in (2, 16):
                team = median_ms(lambda: e.plan_grid_team(spec, walls, None, teams=Teams(size, 0.1), reserve=1, start=start, goal=goal,
                                                          layer_steps=10, layers=T, max_waypoints=32, clearance=False))
                print(f"G = {G:3d}, T = {T:2d}, teams of {size:2d}: time plan (16 shared fields) {alone:.2f} ms, team plan ({n} fields) {team:.2f} ms")
    e.close()


if __name__ == "__main__":
    main()
