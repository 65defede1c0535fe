#!/usr/bin/env python3
"""Wall time of the moving specification monitor at 4096 robots x 1000 steps, point 2x64 (profiles/r33/spec_moving.txt, DESIGN
4.11.4), in the manner of scratch/spec_time.py and scratch/spec_nested_time.py.

  python scratch/spec_moving_time.py                 the table below
  python scratch/spec_moving_time.py --kernel-only   a few monitor calls per leg and nothing else: the program of the one
                                                     `rocprofv3 --kernel-trace --stats` run that gives the kernels' own times
The specification is spec_time.py's (5 clauses over 22 regions) with its 16 hazard boxes replaced by 16 circling hazards (F = 126
frames of dt = 0.05, frame_steps = 1, loop; one shared scene) and one more clause, always(apart(0.05)) in teams of 4.  Legs, in one
process, alternating call by call, 10 rounds after 2 of warm-up, medians: the flat specification (k_spec_monitor), the nested one
at h = 0 (k_spec_monitor_nested), the moving one (k_spec_monitor_moving), and the moving one with its hazards frozen in frame 0
(F = 1: the same kernel without a restage, which prices the restage).  Each is PPOEngine.spec_monitor on one follow call's path:
upload, kernel, download of the state.  goal_rules.spec_fold in NumPy on the same path: one call.  Every timed call ends in a
device synchronise (the entry points are synchronous); clock: perf_counter."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scratch"))
from spec_nested_time import nested_spec, same  # noqa: E402
from spec_time import N, STEPS, make_spec, setup, timed  # noqa: E402

ROUNDS, WARMUP, FRAMES = 10, 2, 126


def moving_spec(n_frames=FRAMES):
    from mobrob_amd.envs.goal_rules import MovingHazards, MovingRegions, Regions, Spec, apart, inside, outside
    flat = make_spec()
    rows = flat.regions.table[0]
    static = Regions(np.concatenate([rows[:4], rows[20:]]), [0] * 4 + [1, 1])          # the arena's boxes, the two goal circles
    hz = MovingHazards.circling(rows[4:20, :2], travel=0.3, size=0.1, n_frames=FRAMES, dt=0.05, frame_steps=1, loop=True)
    mv = MovingRegions.from_hazards(hz)
    if n_frames == 1:
        mv = MovingRegions(mv.table[:, :1], mv.kinds)
    reg = MovingRegions.join(static, mv)
    return Spec(reg, [Spec.always(outside(0, 4)), Spec.always(outside(6, 22), a=1), Spec.eventually(inside(4), 0, 500),
                      Spec.until(outside(6, 22), inside(5)), Spec.eventually(inside(4, 6), 500, None), Spec.always(apart(0.05))],
                team_size=4)


def table():
    from mobrob_amd.envs.goal_rules import spec_fold, spec_start
    specs = {"flat (k_spec_monitor)": make_spec(), "nested h = 0": nested_spec(0), f"moving F = {FRAMES}, mates": moving_spec(),
             "moving F = 1, mates": moving_spec(1)}
    print(f"{N} robots x {STEPS} steps, 2x64 engine, point; synchronous calls; median (min .. max) ms of {ROUNDS} alternating rounds")
    e, env, square, start = setup("point")
    path = env.follow(e, start, square, max_steps=STEPS, seed=1, path_stride=1)["path"]
    ts = {k: [] for k in specs}
    for r in range(WARMUP + ROUNDS):
        for k, sp in specs.items():
            t, _ = timed(lambda: e.spec_monitor(sp, path))
            if r >= WARMUP:
                ts[k].append(t)
    flat_ms = 1e3 * float(np.median(ts["flat (k_spec_monitor)"]))
    nested_ms = 1e3 * float(np.median(ts["nested h = 0"]))
    print(f"point: path {path.nbytes / 2 ** 20:.1f} MiB")
    for k, sp in specs.items():
        v = 1e3 * np.array(ts[k])
        got, res = e.spec_monitor(sp, path)
        line = (f"  {k:<24} {np.median(v):9.3f} ({v.min():.3f} .. {v.max():.3f})  x{np.median(v) / flat_ms:.2f} of flat, "
                f"x{np.median(v) / nested_ms:.2f} of nested h = 0; {sp.n_clauses} clauses")
        if k.startswith("moving F = 126"):
            t, want = timed(lambda: spec_fold(spec_start(N, sp), path, sp))
            line += f"; NumPy rule {1e3 * t:.0f} ms, device == rule bit for bit: {same(got, want)}"
        print(line + f"; satisfied {int(res['satisfied'].sum())}")
    e.close()


def kernel_only():
    e, env, square, start = setup("point")
    path = env.follow(e, start, square, max_steps=STEPS, seed=1, path_stride=1)["path"]
    for sp in (make_spec(), nested_spec(0), moving_spec(), moving_spec(1)):   # in the trace: 5 calls per leg, in this order
        for _ in range(5):
            e.spec_monitor(sp, path)
    e.close()


if __name__ == "__main__":
    kernel_only() if "--kernel-only" in sys.argv[1:] else table()
