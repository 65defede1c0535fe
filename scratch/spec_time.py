#!/usr/bin/env python3
"""Wall time of the specification monitor at 4096 robots x 1000 steps, point and doggo 2x64 (profiles/r31/spec.txt).

  python scratch/spec_time.py                 the table below
  python scratch/spec_time.py --kernel-only   a few monitor calls and nothing else: the program of the one
                                              `rocprofv3 --kernel-trace --stats` run that gives k_spec_monitor's own time
Per robot type, in one process, the legs alternate call by call (A B C A B C ...), 20 rounds after 2 of warm-up, medians:
  A  follow_waypoints, path_stride=0          B  the same call with path_stride=1 (the path comes back to the host)
  C  PPOEngine.spec_monitor on B's path: upload, kernel, download of the state
and goal_rules.spec_fold in NumPy on the same path (3 calls).  The specification has 5 clauses over the arena's four boxes, 16 more
boxes and a goal circle.  Every timed call ends in a device synchronise (the entry points are synchronous); clock: perf_counter."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, STEPS, ROUNDS, WARMUP = 4096, 1000, 20, 2


def make_spec():
    from mobrob_amd.envs.goal_rules import Regions, Spec, Walls, inside, outside
    rng = np.random.default_rng(3)
    boxes = np.concatenate([Walls.enclosure(), np.concatenate([rng.uniform(-1.2, 1.2, (16, 2)), rng.uniform(0.05, 0.2, (16, 2))], axis=1)])
    rows = np.concatenate([boxes, [[1.0, 1.0, 0.3, 0.0], [-1.0, -1.0, 0.3, 0.0]]])
    reg = Regions(rows, [0] * 20 + [1, 1])
    return Spec(reg, [Spec.always(outside(0, 4)), Spec.always(outside(4, 20)), Spec.eventually(inside(20), 0, 500),
                      Spec.until(outside(4, 20), inside(21)), Spec.eventually(inside(20, 22), 500, None)])


def setup(robot):
    from mobrob_amd.engine import PPOEngine
    from mobrob_amd.envs.vec_env import DeviceGoalVecEnv
    from mobrob_amd.envs.wrapper import ROBOT_DIMS
    from mobrob_amd.rl_control.init import orthogonal_policy_init
    D, A, P = ROBOT_DIMS[robot]
    e = PPOEngine(obs_dim=D, act_dim=A, n_envs=16, n_steps=16, batch_size=64, n_epochs=1, pi=(64, 64), vf=(64, 64), seed=1)
    e.set_params(orthogonal_policy_init(D, A, (64, 64), (64, 64), 0))
    env = DeviceGoalVecEnv.for_robot(robot, N, time_limit=0)
    square = np.array([[1.0, 1.0], [1.0, -1.0], [-1.0, -1.0], [-1.0, 1.0]], np.float32)
    start = np.random.default_rng(0).uniform(-0.5, 0.5, (N, P)).astype(np.float32)
    return e, env, square, start


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def table():
    from mobrob_amd.envs.goal_rules import spec_fold, spec_result, spec_start
    spec = make_spec()
    print(f"{N} robots x {STEPS} steps, 2x64 engines, {spec.n_clauses} clauses over {spec.regions.max_regions} regions; synchronous calls; "
          f"median (min .. max) ms of {ROUNDS} alternating rounds")
    for robot in ("point", "doggo"):
        e, env, square, start = setup(robot)
        legs = {"A follow path_stride=0": lambda: env.follow(e, start, square, max_steps=STEPS, seed=1),
                "B follow path_stride=1": lambda: env.follow(e, start, square, max_steps=STEPS, seed=1, path_stride=1)}
        path = legs["B follow path_stride=1"]()["path"]
        legs["C spec_monitor (upload + kernel + download)"] = lambda: e.spec_monitor(spec, path)
        ts = {k: [] for k in legs}
        for r in range(WARMUP + ROUNDS):
            for k, fn in legs.items():
                t, _ = timed(fn)
                if r >= WARMUP:
                    ts[k].append(t)
        rule = [timed(lambda: spec_fold(spec_start(N, spec), path, spec)) for _ in range(3)]
        got, res = e.spec_monitor(spec, path)
        same = np.array_equal(got.val.view(np.uint32), rule[0][1].val.view(np.uint32)) and np.array_equal(got.wit, rule[0][1].wit)
        print(f"{robot}: path {path.nbytes / 2 ** 20:.1f} MiB; device fold == NumPy fold bit for bit: {same}; satisfied {int(res['satisfied'].sum())} of {N}")
        for k, v in ts.items():
            v = 1e3 * np.array(v)
            print(f"  {k:<46} {np.median(v):9.3f} ({v.min():.3f} .. {v.max():.3f})")
        v = 1e3 * np.array([t for t, _ in rule])
        print(f"  {'goal_rules.spec_fold (NumPy), 3 calls':<46} {np.median(v):9.1f} ({v.min():.1f} .. {v.max():.1f})")
        a, b, c = (float(np.median(ts[k])) for k in legs)
        print(f"  path round trip of the follow call (B - A): {1e3 * (b - a):.3f} ms = {100 * (b - a) / b:.1f} % of B; monitor call / B: {100 * c / b:.1f} %")
        spec_result(got, spec)
        e.close()


def kernel_only():
    spec = make_spec()
    e, env, square, start = setup("point")
    path = env.follow(e, start, square, max_steps=STEPS, seed=1, path_stride=1)["path"]
    for _ in range(10):
        e.spec_monitor(spec, path)
    e.close()


if __name__ == "__main__":
    kernel_only() if "--kernel-only" in sys.argv[1:] else table()
