#!/usr/bin/env python3
"""Wall time of waypoint-following runs with robot teams at 4096 robots x 1000 steps, doggo 2x64 (profiles/r14/teams.txt).

  python scratch/teams_time.py PARENT_TREE   (a source tree of the parent commit with its built mobrob_amd/libmobrob_ppo.so)
(1) existing calls -- follow plain, with 16 shared hazards, and as the first call of a run -- on the parent tree and on this one,
    alternating parent / this / parent / this: the spread of each library.
(2) on this tree: the team call (team_size 2 and 16) against the same run call without teams in the same process, without and
    with 16 shared hazards, on the tile and (MOBROB_EVAL_PERSISTENT=0, 100 steps) on the per-step path.
Clocks, children and the CLOCKS DISAGREE flag are scratch/hazard_frames_time.py's."""
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hazard_frames_time import N, ROOT, STEPS, clocks, setup, static_scene, times  # noqa: E402


def leg_existing(runs, warmup):
    from mobrob_amd.waypoints import FollowState
    e, env, square, start = setup()
    hz = static_scene(16, 1, np.random.default_rng(3))
    return {"follow": times(lambda: env.follow(e, start, square, max_steps=STEPS, seed=1), runs, warmup),
            "follow M=16": times(lambda: env.follow(e, start, square, max_steps=STEPS, seed=1, hazards=hz), runs, warmup),
            "run": times(lambda: env.follow(e, max_steps=STEPS, seed=1, resume=FollowState(start, square, None, False, 2)), runs, warmup),
            "run M=16": times(lambda: env.follow(e, max_steps=STEPS, seed=1, hazards=hz, resume=FollowState(start, square, None, True, 2)),
                              runs, warmup)}


def leg_teams(runs, warmup):
    from mobrob_amd.envs.goal_rules import Teams
    from mobrob_amd.waypoints import FollowState
    e, env, square, start = setup()
    hz16 = static_scene(16, 1, np.random.default_rng(3))
    out = {}
    for path, steps in (("tile", STEPS), ("per-step", STEPS // 10)):
        if path == "per-step":
            os.environ["MOBROB_EVAL_PERSISTENT"] = "0"
        for hz, tag in ((None, "no hazards"), (hz16, "M=16")):
            out[f"{path} {tag} base"] = times(lambda: env.follow(e, max_steps=steps, seed=1, hazards=hz,
                                                                resume=FollowState(start, square, None, hz is not None, 2)), runs, warmup)
            for G in (2, 16):
                tm = Teams(G, 0.3)
                fn = lambda: env.follow(e, max_steps=steps, seed=1, hazards=hz, teams=tm,   # noqa: E731
                                        resume=FollowState(start, square, None, hz is not None, 2, True))
                r = fn()
                assert r["persistent"] == (path == "tile")
                out[f"{path} {tag} G={G}"] = times(fn, runs, warmup)
                out[f"conflict rate {path} {tag} G={G}"] = float(np.mean(r["conflict_steps"] > 0))
    return out


def child(what, tree, runs, warmup):
    env = dict(os.environ, HAZARD_TIME_TREE=os.path.abspath(tree))
    for k in ("MOBROB_EVAL_PERSISTENT", "MOBROB_PPO_LIB"):
        env.pop(k, None)
    c = subprocess.run([sys.executable, __file__, "--leg", what, str(runs), str(warmup)], capture_output=True, text=True, env=env,
                       timeout=600)
    if c.returncode != 0:
        sys.exit(f"{what} {tree}: exit status {c.returncode}\n{c.stderr[-3000:]}")
    return json.loads(c.stdout.strip().splitlines()[-1])


def main():
    old, runs, warmup = sys.argv[1], 5, 2
    print(f"{N} robots x {STEPS} steps (per-step path: {STEPS // 10}), doggo 2x64; synchronous calls; ms")
    keys = ["follow", "follow M=16", "run", "run M=16"]
    agg = {t: {k: [] for k in keys} for t in (old, ROOT)}
    flags = []
    for tree in (old, ROOT, old, ROOT):
        r = child("existing", tree, runs, warmup)
        for k in keys:
            agg[tree][k] += r[k]["t"]
            flags.append(clocks(r[k]))
    print("(1) existing calls, two alternating children per library: min / median / max")
    for k in keys:
        for tag, tree in (("parent", old), ("branch", ROOT)):
            t = 1e3 * np.array(agg[tree][k])
            print(f"  {k:<13} {tag}  {t.min():8.2f} {np.median(t):8.2f} {t.max():8.2f}")
    h = child("teams", ROOT, runs, warmup)
    print("(2) team calls (branch): median ms, ratio to the run call without teams in the same process, conflict rate")
    for path in ("tile", "per-step"):
        for tag in ("no hazards", "M=16"):
            b = float(np.median(h[f"{path} {tag} base"]["t"]))
            flags.append(clocks(h[f"{path} {tag} base"]))
            for G in (2, 16):
                rec = h[f"{path} {tag} G={G}"]
                m = float(np.median(rec["t"]))
                flags.append(clocks(rec))
                print(f"  {path:<9} {tag:<11} team_size {G:<3} {1e3 * m:8.2f} ms  base {1e3 * b:7.2f} ms  x{m / b:.3f}  "
                      f"conflict rate {h[f'conflict rate {path} {tag} G={G}']:.3f}")
    bad = [f for f in flags if f != "ok"]
    print(f"clocks: {len(flags) - len(bad)} of {len(flags)} legs agree within 5 % on perf_counter, time.time and HIP events")
    for f in bad[:8]:
        print("  " + f)


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--leg":
        fn = leg_existing if sys.argv[2] == "existing" else leg_teams
        print(json.dumps(fn(int(sys.argv[3]), int(sys.argv[4]))))
    else:
        main()
