#!/usr/bin/env python3
"""Wall time of waypoint-following runs with SOLID teams at 4096 robots x 1000 steps, doggo 2x64 (profiles/r30/teams_solid.txt,
DESIGN 4.10.1).

  python scratch/teams_solid_time.py PARENT_TREE   (a source tree of the parent commit with its built mobrob_amd/libmobrob_ppo.so)
(1) existing calls -- follow plain, a run with observational teams of 4, a run with solid walls (the arena and 16 boxes) -- on the
    parent tree and on this one, alternating parent / this / parent / this, 10 calls per child: medians of 20 per library.
(2) on this tree, in one process: solid teams of 2 and of 16 against the SAME call with observational Teams;
(3) the arena and 16 boxes with solid walls and solid teams of 4 against the same scene with solid walls and observational teams;
(4) solid teams of 4 on the per-step path (MOBROB_EVAL_PERSISTENT=0, 100 steps) against observational teams there.
The serial resolve costs up to `size` dependent rounds on the robot lanes.  Clocks, children and the CLOCKS DISAGREE flag are
scratch/hazard_frames_time.py's."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hazard_frames_time import N, ROOT, STEPS, clocks, setup, times  # noqa: E402
from walls_solid_time import scene_boxes  # noqa: E402

SEP = 0.3


def leg_existing(runs, warmup):
    from mobrob_amd.envs.goal_rules import Teams, Walls
    from mobrob_amd.waypoints import FollowState
    e, env, square, start = setup()
    walls = Walls(scene_boxes(20, 1, np.random.default_rng(3)), radius=0.1, indicator=False, solid=True)
    teams = Teams(4, SEP)
    return {"follow": times(lambda: env.follow(e, start, square, max_steps=STEPS, seed=1), runs, warmup),
            "teams of 4": times(lambda: env.follow(e, max_steps=STEPS, seed=1, teams=teams,
                                                   resume=FollowState(start, square, None, False, 2, True)), runs, warmup),
            "solid walls M=20": times(lambda: env.follow(e, max_steps=STEPS, seed=1, walls=walls,
                                                         resume=FollowState(start, square, None, False, 2, walls=walls)), runs, warmup)}


def leg_solid(runs, warmup):
    from mobrob_amd.envs.goal_rules import Teams, Walls
    from mobrob_amd.waypoints import FollowState
    e, env, square, start = setup()
    walls = Walls(scene_boxes(20, 1, np.random.default_rng(3)), radius=0.1, indicator=False, solid=True)
    out = {}
    for path, steps, G, wl in (("tile", STEPS, 2, None), ("tile", STEPS, 16, None), ("tile", STEPS, 4, walls), ("per-step", STEPS // 10, 4, None)):
        if path == "per-step":
            os.environ["MOBROB_EVAL_PERSISTENT"] = "0"
        tag = f"{path} teams of {G}{' + solid walls M=20' if wl is not None else ''}"
        for name, solid in (("base", False), ("solid", True)):
            teams = Teams(G, SEP, solid=solid)
            fn = lambda: env.follow(e, max_steps=steps, seed=1, teams=teams, walls=wl,   # noqa: E731
                                    resume=FollowState(start, square, None, False, 2, teams, None, wl if wl is not None else False))
            r = fn()
            assert r["persistent"] == (path == "tile")
            out[f"{tag} {name}"] = times(fn, runs, warmup)
        out[f"{tag} rates"] = [float(np.mean(r["team_blocked_steps"] > 0)), float(np.mean(r["team_blocked_steps"]) / steps),
                               float(np.mean(r["team_inside_steps"]) / steps), float(np.mean(r["reached"]))]
    return out


def _run(what, tree, runs, warmup):
    import subprocess
    env = dict(os.environ, HAZARD_TIME_TREE=os.path.abspath(tree))
    for k in ("MOBROB_EVAL_PERSISTENT", "MOBROB_PPO_LIB"):
        env.pop(k, None)
    c = subprocess.run([sys.executable, __file__, "--leg", what, str(runs), str(warmup)], capture_output=True, text=True, env=env,
                       timeout=900)
    if c.returncode != 0:
        sys.exit(f"{what} {tree}: exit status {c.returncode}\n{c.stderr[-3000:]}")
    return json.loads(c.stdout.strip().splitlines()[-1])


def main():
    old, runs, warmup = sys.argv[1], 10, 2
    print(f"{N} robots x {STEPS} steps (per-step path: {STEPS // 10}), doggo 2x64; synchronous calls; ms")
    keys = ["follow", "teams of 4", "solid walls M=20"]
    agg = {t: {k: [] for k in keys} for t in (old, ROOT)}
    flags = []
    for tree in (old, ROOT, old, ROOT):
        r = _run("existing", tree, runs, warmup)
        for k in keys:
            agg[tree][k] += r[k]["t"]
            flags.append(clocks(r[k]))
    print("(1) existing calls, two alternating children per library, 20 calls each: min / median / max")
    for k in keys:
        for tag, tree in (("parent", old), ("branch", ROOT)):
            t = 1e3 * np.array(agg[tree][k])
            print(f"  {k:<17} {tag}  {t.min():8.2f} {np.median(t):8.2f} {t.max():8.2f}")
    h = _run("solid", ROOT, 2 * runs, warmup)
    print("(2)-(4) solid teams (branch): median ms of 20, ratio to the same call with observational teams in the same process;"
          " robots ever blocked by a mate / blocked share of steps / inside share of steps / mean waypoints reached")
    for tag in sorted(k[:-5] for k in h if k.endswith(" base")):
        b, w = (float(np.median(h[f"{tag} {x}"]["t"])) for x in ("base", "solid"))
        flags += [clocks(h[f"{tag} base"]), clocks(h[f"{tag} solid"])]
        print(f"  {tag:<38} {1e3 * w:8.2f} ms  observational {1e3 * b:7.2f} ms  x{w / b:.3f}  rates {h[f'{tag} rates']}")
    bad = [f for f in flags if f != "ok"]
    print(f"clocks: {len(flags) - len(bad)} of {len(flags)} legs agree within 5 % on perf_counter, time.time and HIP events")
    for f in bad[:8]:
        print("  " + f)


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--leg":
        fn = leg_existing if sys.argv[2] == "existing" else leg_solid
        print(json.dumps(fn(int(sys.argv[3]), int(sys.argv[4]))))
    else:
        main()
