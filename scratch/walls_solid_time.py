#!/usr/bin/env python3
"""Wall time of waypoint-following runs with SOLID walls at 4096 robots x 1000 steps, doggo 2x64 (profiles/r27/walls_solid.txt,
DESIGN 4.11.1).

  python scratch/walls_solid_time.py PARENT_TREE   (a source tree of the parent commit with its built mobrob_amd/libmobrob_ppo.so)
(1) existing calls -- follow plain, with 16 shared hazards, and as the first call of a run -- on the parent tree and on this one,
    alternating parent / this / parent / this: the spread of each library (scratch/walls_time.py's leg).
(2) on this tree: the run call with solid walls against the SAME call with observational walls, in the same process: shared scenes
    of M = 4, 20 (the arena and 16 boxes), 64 and 1024 walls, 16 per-robot scenes of M = 16, on the tile and
    (MOBROB_EVAL_PERSISTENT=0, 100 steps, M = 64) on the per-step path.  The resolution is serial on the robot's lane: whatever
    M = 1024 costs is what a wide phase would have to beat.
Clocks, children and the CLOCKS DISAGREE flag are scratch/hazard_frames_time.py's."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hazard_frames_time import N, ROOT, STEPS, clocks, setup, times  # noqa: E402
from teams_time import leg_existing  # noqa: E402


def scene_boxes(M, S, rng):
    """S scenes of M boxes spread over the arena the robots move in; M = 20: the reference's enclosure and 16 boxes"""
    from mobrob_amd.envs.goal_rules import Walls
    m = M - 4 if M == 20 else M
    boxes = np.concatenate([rng.uniform(-2.5, 2.5, (S, m, 2)), rng.uniform(0.01, 0.15, (S, m, 2))], axis=-1)
    if M == 20:
        boxes = np.concatenate([np.broadcast_to(Walls.enclosure(5.6, 0.265), (S, 4, 4)), boxes], axis=1)
    return boxes if S > 1 else boxes[0]


def leg_solid(runs, warmup):
    from mobrob_amd.envs.goal_rules import Walls
    from mobrob_amd.waypoints import FollowState
    e, env, square, start = setup()
    rng = np.random.default_rng(3)
    out = {}
    cases = [("tile", STEPS, "shared", M) for M in (4, 20, 64, 1024)] + [("tile", STEPS, "per-robot", 16), ("per-step", STEPS // 10, "shared", 64)]
    for path, steps, kind, M in cases:
        if path == "per-step":
            os.environ["MOBROB_EVAL_PERSISTENT"] = "0"
        S = 1 if kind == "shared" else 16
        scene = None if S == 1 else (np.arange(N) % S).astype(np.int32)
        boxes = scene_boxes(M, S, rng)
        tag = f"{path} {kind} M={M}"
        for name, solid in (("base", False), ("solid", True)):
            walls = Walls(boxes, scene=scene, radius=0.1, indicator=False, solid=solid)
            fn = lambda: env.follow(e, max_steps=steps, seed=1, walls=walls,   # noqa: E731
                                    resume=FollowState(start, square, None, False, 2, walls=walls))
            r = fn()
            assert r["persistent"] == (path == "tile")
            out[f"{tag} {name}"] = times(fn, runs, warmup)
        out[f"{tag} rates"] = [float(np.mean(r["wall_blocked_steps"] > 0)), float(np.mean(r["wall_blocked_steps"]) / steps),
                               float(np.mean(r["reached"]))]
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
    old, runs, warmup = sys.argv[1], 5, 2
    print(f"{N} robots x {STEPS} steps (per-step path: {STEPS // 10}), doggo 2x64; synchronous calls; ms")
    keys = ["follow", "follow M=16", "run", "run M=16"]
    agg = {t: {k: [] for k in keys} for t in (old, ROOT)}
    flags = []
    for tree in (old, ROOT, old, ROOT):
        r = _run("existing", tree, runs, warmup)
        for k in keys:
            agg[tree][k] += r[k]["t"]
            flags.append(clocks(r[k]))
    print("(1) existing calls, two alternating children per library: min / median / max")
    for k in keys:
        for tag, tree in (("parent", old), ("branch", ROOT)):
            t = 1e3 * np.array(agg[tree][k])
            print(f"  {k:<13} {tag}  {t.min():8.2f} {np.median(t):8.2f} {t.max():8.2f}")
    h = _run("solid", ROOT, runs, warmup)
    print("(2) solid walls (branch): median ms, ratio to the same call with observational walls in the same process;"
          " robots ever blocked / blocked share of steps / mean waypoints reached")
    for tag in sorted(k[:-5] for k in h if k.endswith(" base")):
        b, w = (float(np.median(h[f"{tag} {x}"]["t"])) for x in ("base", "solid"))
        flags += [clocks(h[f"{tag} base"]), clocks(h[f"{tag} solid"])]
        print(f"  {tag:<26} {1e3 * w:8.2f} ms  observational {1e3 * b:7.2f} ms  x{w / b:.3f}  rates {h[f'{tag} rates']}")
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
