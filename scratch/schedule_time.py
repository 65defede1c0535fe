#!/usr/bin/env python3
"""Wall time of waypoint-following runs with timed waypoints at 4096 robots x 1000 steps, doggo 2x64 (profiles/r15/schedule.txt,
DESIGN 4.8.2).

  python scratch/schedule_time.py PARENT_TREE   (a source tree of the parent commit with its built mobrob_amd/libmobrob_ppo.so)
(a) existing calls -- follow plain, as the first call of a run, and the run with teams of 4 -- on the parent tree and on this one,
    alternating parent / this / parent / this: the spread of each library.
(b) on this tree: the scheduled call with all-zero releases against the same run call without a schedule, in the same process.
(c) the scheduled call with a stagger of 25 steps per team member, without and with teams of 4.
Clocks, children and the CLOCKS DISAGREE flag are scratch/hazard_frames_time.py's."""
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hazard_frames_time import N, ROOT, STEPS, clocks, setup, times  # noqa: E402


def leg_existing(runs, warmup):
    from mobrob_amd.envs.goal_rules import Teams
    from mobrob_amd.waypoints import FollowState
    e, env, square, start = setup()
    tm = Teams(4, 0.3)
    return {"follow": times(lambda: env.follow(e, start, square, max_steps=STEPS, seed=1), runs, warmup),
            "run": times(lambda: env.follow(e, max_steps=STEPS, seed=1, resume=FollowState(start, square, None, False, 2)), runs, warmup),
            "teams": times(lambda: env.follow(e, max_steps=STEPS, seed=1, teams=tm, resume=FollowState(start, square, None, False, 2, True)),
                           runs, warmup)}


def leg_schedule(runs, warmup):
    from mobrob_amd.envs.goal_rules import Schedule, Teams
    from mobrob_amd.waypoints import FollowState
    e, env, square, start = setup()
    K = np.shape(square)[-2]
    zero = Schedule(np.zeros((N, K), np.int32))
    stagger = Schedule((25 * (np.arange(N) % 4))[:, None] + np.zeros((N, K), np.int32))
    tm = Teams(4, 0.3)
    out = {"base": times(lambda: env.follow(e, max_steps=STEPS, seed=1, resume=FollowState(start, square, None, False, 2)), runs, warmup)}
    for tag, sc, teams in (("zero", zero, None), ("stagger", stagger, None), ("stagger teams", stagger, tm)):
        fn = lambda: env.follow(e, max_steps=STEPS, seed=1, schedule=sc, teams=teams,   # noqa: E731
                                resume=FollowState(start, square, None, False, 2, teams is not None, sc))
        r = fn()
        assert r["persistent"] is True
        out[tag] = times(fn, runs, warmup)
        out["hold steps " + tag] = float(np.mean(r["hold_steps"]))
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
    print(f"{N} robots x {STEPS} steps, doggo 2x64; synchronous calls; ms")
    keys = ["follow", "run", "teams"]
    agg = {t: {k: [] for k in keys} for t in (old, ROOT)}
    flags = []
    for tree in (old, ROOT, old, ROOT):
        r = child("existing", tree, runs, warmup)
        for k in keys:
            agg[tree][k] += r[k]["t"]
            flags.append(clocks(r[k]))
    print("(a) existing calls, two alternating children per library: min / median / max")
    for k in keys:
        for tag, tree in (("parent", old), ("branch", ROOT)):
            t = 1e3 * np.array(agg[tree][k])
            print(f"  {k:<8} {tag}  {t.min():8.2f} {np.median(t):8.2f} {t.max():8.2f}")
    h = child("schedule", ROOT, runs, warmup)
    b = float(np.median(h["base"]["t"]))
    print("(b), (c) scheduled calls (branch): median ms, ratio to the run call without a schedule in the same process, mean hold steps")
    for tag in ("zero", "stagger", "stagger teams"):
        m = float(np.median(h[tag]["t"]))
        flags.append(clocks(h[tag]))
        print(f"  {tag:<14} {1e3 * m:8.2f} ms  base {1e3 * b:7.2f} ms  x{m / b:.3f}  hold steps {h['hold steps ' + tag]:.1f}")
    bad = [f for f in flags if f != "ok"]
    print(f"clocks: {len(flags) - len(bad)} of {len(flags)} legs agree within 5 % on perf_counter, time.time and HIP events")
    for f in bad[:8]:
        print("  " + f)


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--leg":
        fn = leg_existing if sys.argv[2] == "existing" else leg_schedule
        print(json.dumps(fn(int(sys.argv[3]), int(sys.argv[4]))))
    else:
        main()
