"""CPU: timed waypoints (goal_rules.Schedule / schedule_fold) and schedules on the host loop of mobrob_amd.waypoints.

The job of the GPU tests is built here (`job`) and held to conditions on the host rule alone: n = 20 robots, K = 3 waypoints,
T = 64 steps, split 32 + 32.  Robots i % 4 == 0 have all releases 0 (no hold); i % 4 == 1 hold at home for 10 steps; i % 4 == 2
reach waypoint 0 long before waypoint 1 is released at T/2 - 1, T/2 or T/2 + 1 and are still under way when waypoint 2 is released
at step 36; i % 4 == 3 have waypoint 1 released at step 5, before they arrive at waypoint 0, and hold at waypoint 1 until step 50."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from mobrob_amd.envs.goal_rules import SCHED_START, Schedule, goal_distance32, schedule_fold
from mobrob_amd.waypoints import FollowState, follow_waypoints, follow_with_replanning
from tests.test_teams_cpu import _GoToGoal

N, K, T = 20, 3, 64
SPLIT = (T // 2, T // 2)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def job(P=2, n=N):
    """-> start [n][P], waypoints [n][K][P], counts [n], release [n][K] (see the module docstring)"""
    rng = np.random.default_rng(11)
    start = rng.uniform(-1.2, 1.2, (n, P))
    wp = np.zeros((n, K, P))
    at = start
    for k in range(K):
        u = rng.standard_normal((n, P))
        at = np.clip(at + (0.8 if k == 0 else 0.6) * u / np.linalg.norm(u, axis=1, keepdims=True), -2.5, 2.5)
        wp[:, k] = at
    nw = np.full(n, K, np.int32)
    nw[8] = 0                                                   # a robot without waypoints: never steps, never holds
    nw[12] = 2                                                  # a short row: its third release is ignored
    rel = np.zeros((n, K), np.int32)
    for i in range(n):
        if i % 4 == 1:
            rel[i] = (10, 0, 0)
        elif i % 4 == 2:
            rel[i] = (0, T // 2 - 1 + (i // 4) % 3, 36)
        elif i % 4 == 3:
            rel[i] = (0, 5, 50)
    return start.astype(np.float32), wp.astype(np.float32), nw, rel


def test_schedule_rule_by_hand():
    wp = np.array([[[1.0, 0.0], [2.0, 0.0], [3.0, 0.0]], [[0.0, 1.0], [0.0, 2.0], [0.0, 3.0]]], np.float32)
    home = np.array([[9.0, 9.0], [8.0, 8.0]], np.float32)
    nw = np.array([3, 2])
    rel = np.array([[4, 2, 7], [0, 5, 99]])                     # robot 0: waypoint 1 released before waypoint 0 (never holds)
    hold = lambda k, g: Schedule.holding(rel, nw, np.array(k), g).tolist()          # noqa: E731
    goal = lambda k, g: Schedule.goal(rel, home, wp, nw, np.array(k), g).tolist()   # noqa: E731
    assert hold([0, 0], 3) == [True, False] and hold([0, 0], 4) == [False, False]
    assert goal([0, 0], 3) == [[9.0, 9.0], [0.0, 1.0]]          # k = 0 holds at home
    assert goal([0, 0], 4) == [[1.0, 0.0], [0.0, 1.0]]
    assert hold([1, 1], 4) == [False, True] and goal([1, 1], 4) == [[2.0, 0.0], [0.0, 1.0]]   # anchor: the previous waypoint
    assert hold([2, 1], 6) == [True, False] and goal([2, 1], 6) == [[2.0, 0.0], [0.0, 2.0]]
    assert hold([3, 2], 0) == [False, False]                    # k = nwp: no hold (robot 1's third release is not in use) ...
    assert goal([3, 2], 0) == [[3.0, 0.0], [0.0, 2.0]]          # ... and the last waypoint is kept
    late = Schedule.lateness(rel, np.array([[6, 9, -1], [1, -1, -1]]))
    assert np.array_equal(late, [[2, 7, np.nan], [1, np.nan, np.nan]], equal_nan=True)
    r, h = Schedule([3, 4]).for_robots(2, 3, home)
    assert np.array_equal(r, [[3, 4, 0], [3, 4, 0]]) and r.dtype == np.int32 and np.array_equal(h, home)
    for bad in ([-1, 0], [0.5, 1.0], [[True]], np.zeros((1, 1, 1), int), []):
        with pytest.raises(ValueError):
            Schedule(bad)
    with pytest.raises(ValueError):
        Schedule([0], home=[[np.inf, 0.0]])
    with pytest.raises(ValueError):
        Schedule([0, 0, 0, 0]).for_robots(2, 3, home)           # more releases than waypoint slots
    with pytest.raises(ValueError):
        Schedule(np.zeros((3, 2), int)).for_robots(2, 3, home)


def test_schedule_fold_and_the_device_s_distance():
    assert goal_distance32([[3.0, 4.0]], [[0.0, 0.0]])[0] == 5.0 and goal_distance32([[1, 2, 3]], [[1, 2, 3]])[0] == 0.0
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal((500, 3)).astype(np.float32), rng.standard_normal((500, 3)).astype(np.float32)
    d64 = np.linalg.norm(a.astype(np.float64) - b.astype(np.float64), axis=1)
    assert np.all(np.abs(goal_distance32(a, b) - d64) <= 4 * 2.0 ** -24 * np.maximum(d64, 1.0))    # 3 differences, 3 fmas, 1 root
    anchor, pos = np.zeros((3, 2, 2), np.float32), np.zeros((3, 2, 2), np.float32)
    pos[:, 0, 0] = (0.25, 0.5, 0.125)
    pos[:, 1, 0] = 7.0
    rec = schedule_fold(np.tile(SCHED_START, (2, 1)), anchor, pos, [[True, False], [True, False], [False, False]])
    assert np.array_equal(rec, [[2, 0.5], [0, np.nan]], equal_nan=True)
    again = schedule_fold(rec, anchor[:1], pos[2:], [[True, True]])                               # continued, never re-summed
    assert np.array_equal(again, [[3, 0.5], [1, 7.0]])
    with pytest.raises(ValueError):
        schedule_fold(np.zeros((3, 2)), anchor, pos, np.zeros((3, 2), bool))


def _host(P=2, split=(T,), release=True, **kw):
    start, wp, nw, rel = job(P)
    pol, name = _GoToGoal("point" if P == 2 else "drone"), "point" if P == 2 else "drone"
    r = None
    for i, steps in enumerate(split):
        first = dict(start=start, waypoints=wp, n_waypoints=nw) if i == 0 else dict(state=r["state"])
        r = follow_waypoints(pol, name, max_steps=steps, seed=1, schedule=Schedule(rel) if release else None, **first, **kw)
    return r, (start, wp, nw, rel)


@pytest.mark.parametrize("P", [2, 3])
def test_the_setup_on_the_host_rule(P):
    """conditions on the inputs of the GPU tests, met by the host rule alone"""
    r, (start, wp, nw, rel) = _host(P)
    holds, arr = r["hold_steps"], r["arrival"]
    assert np.sum(holds >= 1) >= N // 4 and np.sum(holds == 0) >= N // 4, holds
    timed = [(i, k) for i in range(N) for k in range(1, nw[i]) if rel[i, k] > 0 and arr[i, k - 1] > 0]
    assert any(arr[i, k - 1] < rel[i, k] for i, k in timed), "a robot that arrives before its next release"
    assert any(rel[i, k] <= arr[i, k - 1] for i, k in timed), "a release that passes before the robot arrives"
    home_hold = (rel[:, 0] > 0) & (nw > 0)
    assert np.any(home_hold) and np.all(holds[home_hold] >= rel[home_hold, 0])                    # holds at home
    assert np.all(r["hold_drift"][home_hold & (holds == rel[:, 0])] == 0.0)                       # ... exactly there
    used = rel[np.arange(K)[None, :] < nw[:, None]]
    bounds = np.cumsum((0,) + SPLIT)
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        assert np.any((used > lo) & (used < hi)), (lo, hi)                                        # a release strictly inside each call
    assert {T // 2 - 1, T // 2, T // 2 + 1} <= set(used.tolist())                                 # on, just before, just after the boundary
    assert holds[8] == 0 and r["steps"][8] == 0 and np.isnan(r["hold_drift"][8])
    # a hold step is a step: it counts, it earns nothing, and it is no arrival
    i = int(np.nonzero(home_hold)[0][0])
    assert r["steps"][i] >= holds[i] and arr[i, 0] > rel[i, 0]
    assert np.array_equal(np.isnan(r["lateness"]), arr < 0) and np.nanmin(r["lateness"][:, 0]) >= 1


@pytest.mark.parametrize("split", [SPLIT, (1, T - 1), (T // 2 - 1, 2, T // 2 - 1)])
def test_a_split_run_is_the_unsplit_run(split):
    one, _ = _host()
    got, _ = _host(split=split)
    for f in ("state", "robot", "arrival", "leg_used", "status", "sched", "release", "home", "step0"):
        assert np.array_equal(getattr(one["state"], f), getattr(got["state"], f), equal_nan=True), (split, f)
    for k in ("hold_steps", "hold_drift", "lateness", "reward_sum", "steps"):
        assert np.array_equal(one[k], got[k], equal_nan=True), (split, k)


def test_an_all_zero_schedule_changes_nothing():
    start, wp, nw, rel = job()
    pol = _GoToGoal()
    kw = dict(max_steps=T, seed=1, path_stride=4, leg_steps=20)
    plain = follow_waypoints(pol, "point", start, wp, nw, **kw)
    zero = follow_waypoints(pol, "point", start, wp, nw, schedule=Schedule(np.zeros_like(rel)), **kw)
    assert set(zero) == set(plain) | {"hold_steps", "hold_drift", "lateness"}
    for k in plain:
        if k == "state":
            for f in ("state", "robot", "arrival", "leg_used", "status", "step0"):
                assert np.array_equal(getattr(plain[k], f), getattr(zero[k], f), equal_nan=True), f
        elif k not in ("trace", "persistent"):
            assert np.array_equal(plain[k], zero[k], equal_nan=True), k
    assert np.array_equal(zero["state"].sched, np.tile(SCHED_START, (N, 1)), equal_nan=True)
    assert np.any(plain["status"] == 1)


def test_replan_with_release():
    r, (start, wp, nw, rel) = _host(split=(T // 2,))
    st = r["state"]
    before = st.copy()
    assert before.sched is not st.sched and np.array_equal(before.release, st.release)
    rows = np.array([1, 6])
    new = st.positions[rows][:, None, :] + np.array([[[0.5, 0.0]], [[0.0, 0.5]]], np.float32)
    st.replan(rows, new, release=np.array([[40], [0]]))
    assert np.all(st.robot[rows, 2] == 0) and np.all(st.arrival[rows] == -1) and np.all(st.leg_used[rows] == 0)
    assert np.array_equal(st.home[rows], before.state[rows, :2].astype(np.float32))               # home: where the robot is
    assert np.array_equal(st.release[rows], [[40, 0, 0], [0, 0, 0]]) and np.array_equal(st.n_waypoints[rows], [1, 1])
    keep = np.setdiff1d(np.arange(N), rows)
    for f in ("release", "home", "arrival", "waypoints"):
        assert np.array_equal(getattr(st, f)[keep], getattr(before, f)[keep]), f
    for f in ("sched", "state"):
        assert np.array_equal(getattr(st, f), getattr(before, f), equal_nan=True), f                # carried
    assert np.array_equal(st.robot[:, :2], before.robot[:, :2])
    st.replan([2], new[:1])                                                                       # no release: released at once
    assert np.array_equal(st.release[2], [0, 0, 0]) and np.array_equal(st.home[2], before.state[2, :2].astype(np.float32))
    r2 = follow_waypoints(_GoToGoal(), "point", max_steps=T // 2, seed=1, state=st, schedule=Schedule(rel))
    assert r2["hold_steps"][1] - r["hold_steps"][1] == 40 - T // 2 and r2["arrival"][1, 0] > 40 and 0 < r2["arrival"][6, 0]
    # a run without a schedule: replan is what it was, and release= is refused
    plain = FollowState(start, wp, nw)
    twin = plain.copy().replan(rows, new)
    assert twin.release is None and twin.sched is None and np.array_equal(twin.waypoints[rows, :1], new.astype(np.float32))
    with pytest.raises(ValueError):
        plain.replan(rows, new, release=[[1], [1]])
    with pytest.raises(ValueError):                                                               # scheduled in every call or in none
        follow_waypoints(_GoToGoal(), "point", max_steps=5, state=plain, schedule=Schedule(rel))
    with pytest.raises(ValueError):
        follow_waypoints(_GoToGoal(), "point", max_steps=5, state=r["state"])
    with pytest.raises(TypeError):
        follow_waypoints(_GoToGoal(), "point", start, wp, nw, max_steps=5, schedule=rel)
    out = follow_with_replanning(_GoToGoal(), "point", start, wp, lambda pos, status, reached: {}, horizon=T // 2, rounds=2,
                                 n_waypoints=nw, seed=1, schedule=Schedule(rel))
    one, _ = _host()
    assert np.array_equal(out["state"].sched, one["state"].sched, equal_nan=True)


def test_the_symbol_and_the_struct_layout(tmp_path):
    """the new entry point is exported and bound, and mobrob_follow_schedule_t is laid out as the ctypes mirror"""
    import __graft_entry__
    __graft_entry__.build()
    from mobrob_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "mobrob_ppo_follow_waypoints_scheduled") and "mobrob_ppo_follow_waypoints_scheduled" in _lib.SYMBOLS
    assert len(_lib.SYMBOLS["mobrob_ppo_follow_waypoints_scheduled"][1]) == len(_lib.SYMBOLS["mobrob_ppo_follow_waypoints_teams"][1]) + 2
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "mobrob_ppo.h"\nint main(void) {\n'
            '  printf("%zu %zu %zu\\n", sizeof(mobrob_follow_schedule_t), offsetof(mobrob_follow_schedule_t, release),\n'
            '         offsetof(mobrob_follow_schedule_t, home));\n  return 0;\n}\n')
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(prog)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _lib.FollowScheduleC
    assert out == [ctypes.sizeof(S), S.release.offset, S.home.offset]
