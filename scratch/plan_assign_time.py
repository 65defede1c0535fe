"""Times one mobrob_ppo_plan_assign call beside mobrob_ppo_plan_grid_team of the same run (what assignment adds to a team plan) and
beside a mobrob_ppo_plan_grid call with as many fields, one per robot (what k_plan_assign_cost saves by keeping its fields in LDS: that
call writes n fields of G * G ints to memory), the shape of scratch/plan_team_rounds_time.py: 4096 robots with a goal each, the enclosure
plus 16 boxes, G in {64, 128}, teams of 2 and 16, both objectives.  Host clock around a call that ends in a stream synchronise, `warm`
warm-up calls, median of `runs`.  Beside the times: the teams whose pairing changed and the total cost before and after.  Prints one
line per case; record them in profiles/r25/plan_assign.txt.
    python scratch/plan_assign_time.py [runs [warm [G,G.. [T]]]]"""
import sys

import numpy as np

from mobrob_amd.engine import PPOEngine
from mobrob_amd.envs.goal_rules import GridSpec, Teams, Walls
from scratch.plan_team_rounds_time import median_ms


def main():
    runs, warm = (int(sys.argv[1]) if len(sys.argv) > 1 else 10), (int(sys.argv[2]) if len(sys.argv) > 2 else 2)
    grids = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [64, 128]
    T = int(sys.argv[4]) if len(sys.argv) > 4 else 16
    rng = np.random.default_rng(0)
    n = 4096
    boxes = np.concatenate([Walls.enclosure(3.6, 0.2), np.column_stack([rng.uniform(-1.3, 1.3, (16, 2)), rng.uniform(0.05, 0.2, (16, 2))])])
    walls = Walls(boxes, radius=0.05)
    start = rng.uniform(-1.5, 1.5, (n, 2)).astype(np.float32)
    goal = rng.uniform(-1.5, 1.5, (n, 2)).astype(np.float32)
    e = PPOEngine(obs_dim=8, act_dim=2, n_envs=16, n_steps=8, batch_size=64, n_epochs=1, pi=(64, 64), vf=(64, 64), seed=0)
    for G in grids:
        spec = GridSpec(2.0, G)
        fields = median_ms(lambda: e.plan_grid(spec, walls, None, start=start, goal=goal, max_waypoints=32), runs, warm)
        n_fields = len(e.plan_grid(spec, walls, None, start=start, goal=goal, max_waypoints=32)["field_goal_cell"])
        print(f"G = {G:3d}: plan_grid with {n_fields} fields written out {fields:.2f} ms", flush=True)
        for size in (2, 16):
            teams = Teams(size, 0.1)
            plain = median_ms(lambda: e.plan_grid_team(spec, walls, None, teams=teams, reserve=1, start=start, goal=goal, layer_steps=10, layers=T,
                                                       max_waypoints=32, clearance=False), runs, warm)
            for objective in ("sum", "makespan"):
                ms = median_ms(lambda: e.plan_assign(spec, walls, None, teams=teams, start=start, goal=goal, objective=objective), runs, warm)
                out = e.plan_assign(spec, walls, None, teams=teams, start=start, goal=goal, objective=objective)
                print(f"G = {G:3d}, teams of {size:2d}, {objective:8s}: assign {ms:.2f} ms, team plan (T = {T}) {plain:.2f} ms ({ms / plain:.2f} x of it), "
                      f"plan_grid {fields:.2f} ms ({ms / fields:.2f} x of it); {int(out['assign_changed'].sum())} of {n // size} teams changed, "
                      f"total {int(out['assign_identity_total'].sum())} -> {int(out['assign_total'].sum())}, status 3: "
                      f"{int((out['assign_status'] == 3).sum())}", flush=True)
    e.close()


if __name__ == "__main__":
    main()
