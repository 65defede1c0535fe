#!/usr/bin/env python3
"""Wall time of the nested specification monitor at 4096 robots x 1000 steps, point and doggo 2x64 (profiles/r32/spec_nested.txt,
DESIGN 4.11.3), in the manner of scratch/spec_time.py.

  python scratch/spec_nested_time.py                 the table below
  python scratch/spec_nested_time.py --kernel-only   a few monitor calls per hold and nothing else: the program of the one
                                                     `rocprofv3 --kernel-trace --stats` run that gives the kernels' own times
The specification is spec_time.py's (5 clauses over 22 regions) with its first `eventually` replaced by `stay(h)` and its second
`always` by `recur(h)`, for h in 0, 16, 64, 255.  Per robot type, in one process, the legs alternate call by call (flat, h = 0, 16,
64, 255, flat, ...), 10 rounds after 2 of warm-up, medians: PPOEngine.spec_monitor on one follow call's path -- upload, kernel,
download of the state and, for the nested legs, of the tail.  goal_rules.spec_fold in NumPy on the same path: one call per leg, point
only.  Every timed call ends in a device synchronise (the entry points are synchronous); clock: perf_counter."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scratch"))
from spec_time import N, STEPS, make_spec, setup, timed  # noqa: E402

ROUNDS, WARMUP, HOLDS = 10, 2, (0, 16, 64, 255)


def nested_spec(h):
    from mobrob_amd.envs.goal_rules import Spec
    flat = make_spec()
    cl = list(flat.clauses)
    cl[1] = Spec.recur(cl[1][3], h, cl[1][1], None)          # always outside the 16 boxes -> in every h + 1 samples outside them once
    cl[2] = Spec.stay(cl[2][3], h, cl[2][1], cl[2][2])       # eventually inside the goal circle in [0, 500] -> for h + 1 samples
    return Spec(flat.regions, cl)


def same(a, b):
    return all(np.array_equal(getattr(a, k).view(np.uint32), getattr(b, k).view(np.uint32)) for k in ("val", "wit", "tail"))


def table():
    from mobrob_amd.envs.goal_rules import spec_fold, spec_start
    specs = {"flat (k_spec_monitor)": make_spec()}
    specs.update({f"nested h = {h}": nested_spec(h) for h in HOLDS})
    print(f"{N} robots x {STEPS} steps, 2x64 engines, 5 clauses over 22 regions; synchronous calls; median (min .. max) ms of {ROUNDS} "
          f"alternating rounds")
    for robot in ("point", "doggo"):
        e, env, square, start = setup(robot)
        path = env.follow(e, start, square, max_steps=STEPS, seed=1, path_stride=1)["path"]
        ts = {k: [] for k in specs}
        for r in range(WARMUP + ROUNDS):
            for k, sp in specs.items():
                t, _ = timed(lambda: e.spec_monitor(sp, path))
                if r >= WARMUP:
                    ts[k].append(t)
        flat_ms = 1e3 * float(np.median(ts["flat (k_spec_monitor)"]))
        print(f"{robot}: path {path.nbytes / 2 ** 20:.1f} MiB")
        for k, sp in specs.items():
            v = 1e3 * np.array(ts[k])
            got, res = e.spec_monitor(sp, path)
            line = f"  {k:<24} {np.median(v):9.3f} ({v.min():.3f} .. {v.max():.3f})  x{np.median(v) / flat_ms:.2f} of flat; tail {got.tail.nbytes / 2 ** 20:.2f} MiB"
            if robot == "point":
                t, want = timed(lambda: spec_fold(spec_start(N, sp), path, sp))
                line += f"; NumPy rule {1e3 * t:.0f} ms, device == rule bit for bit: {same(got, want)}"
            print(line + f"; satisfied {int(res['satisfied'].sum())}")
        e.close()


def kernel_only():
    e, env, square, start = setup("point")
    path = env.follow(e, start, square, max_steps=STEPS, seed=1, path_stride=1)["path"]
    for sp in [make_spec()] + [nested_spec(h) for h in HOLDS]:   # in the trace: 5 calls of k_spec_monitor, then 5 per hold in this order
        for _ in range(5):
            e.spec_monitor(sp, path)
    e.close()


if __name__ == "__main__":
    kernel_only() if "--kernel-only" in sys.argv[1:] else table()
