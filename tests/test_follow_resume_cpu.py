"""CPU: resumable waypoint following on the host loop (mobrob_amd.waypoints): a run split into calls ends where one call ends,
leg budgets and status, FollowState.replan, follow_with_replanning, input checks, and examples/follow.py --horizon / --leg-steps
up to the point where a device is needed."""
import ctypes
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from mobrob_amd.envs.wrapper import get_env
from mobrob_amd.waypoints import (FINISHED, GOING, NO_WAYPOINTS, STALLED, FollowState, follow_waypoints,
                                  follow_with_replanning)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "examples", "follow.py")
SQUARE = np.array([[1.0, 1.0], [1.0, -1.0], [-1.0, -1.0], [-1.0, 1.0]])
FAR = np.array([5.0, 5.0])          # outside +-extent (3): never reached


class _Scripted:
    """predict = a command towards the goal plus a term in the observation's noise features: the action depends on the noise
    drawn for the step, so a split that drew other noise would show."""

    def __init__(self, env_name="point"):
        env = get_env(env_name)
        self.P = env.env.pos_dim
        self.A = np.linalg.pinv(env.env._mix)

    def predict(self, obs, deterministic=True):
        o = np.asarray(obs, np.float64)
        return np.clip(self.A @ o[:self.P] + 0.3 * o[3 * self.P:3 * self.P + self.A.shape[0]], -1.0, 1.0), None


def _carried(r):
    s = r["state"]
    d = {"state": s.state, "robot": s.robot, "arrival": s.arrival, "leg_used": s.leg_used, "status": s.status,
         "step0": np.array(s.step0)}
    if s.hazard is not None:
        d["hazard"] = s.hazard
    return d


def _job(n=5):
    starts = np.random.default_rng(3).uniform(-0.5, 0.5, (n, 2))
    wp = np.broadcast_to(SQUARE, (n, 4, 2)).copy()
    wp[1, 1] = FAR                                  # robot 1: second waypoint unreachable
    nw = np.array([4, 4, 0, 2, 4][:n])
    return starts, wp, nw


@pytest.mark.parametrize("leg_steps", [0, 45])
@pytest.mark.parametrize("split", [(1, 119), (40, 80), (119, 1), (40, 40, 40)])
def test_a_split_run_ends_where_one_call_ends(split, leg_steps):
    from mobrob_amd.envs.goal_rules import Hazards
    starts, wp, nw = _job()
    hz = Hazards(np.array([[0.8, 0.8], [1.0, 0.0], [-0.5, -1.0]]), 0.35, indicator=False)
    pol = _Scripted()
    one = follow_waypoints(pol, "point", starts, wp, nw, max_steps=120, seed=7, hazards=hz, leg_steps=leg_steps)
    r = None
    for i, steps in enumerate(split):
        r = follow_waypoints(pol, "point", starts if i == 0 else None, wp if i == 0 else None, nw if i == 0 else None,
                             max_steps=steps, seed=7, hazards=hz, leg_steps=leg_steps, state=None if i == 0 else r["state"])
    a, b = _carried(one), _carried(r)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    for k in ("arrival", "reached", "steps", "reward_sum", "final_distance", "cost_sum", "violation_steps", "first_violation",
              "min_clearance", "status"):
        assert np.array_equal(one[k], r[k], equal_nan=True), k
    # not vacuous: arrivals in every third of the run, and with the budget a stalled and a finished robot
    arr = one["arrival"][one["arrival"] > 0]
    assert np.any(one["cost_sum"] > 0)
    if not leg_steps:
        assert all(np.any((arr > lo) & (arr <= lo + 40)) for lo in (0, 40, 80))
    else:
        assert np.any(one["status"] == STALLED) and np.any(one["status"] == FINISHED)


def test_the_noise_is_drawn_per_global_step():
    starts, wp, nw = _job()
    pol = _Scripted()
    a = follow_waypoints(pol, "point", starts, wp, nw, max_steps=30, seed=7)
    b = follow_waypoints(pol, "point", starts, wp, nw, max_steps=30, seed=8)
    assert not np.array_equal(a["reward_sum"], b["reward_sum"])
    st = a["state"].copy()
    st.step0 += 1                                   # the same robots, another global step: other noise
    c = follow_waypoints(pol, "point", max_steps=30, seed=7, state=a["state"])
    d = follow_waypoints(pol, "point", max_steps=30, seed=7, state=st)
    assert not np.array_equal(c["reward_sum"], d["reward_sum"])


def test_budget_and_status_on_env_wrapper():
    """Robot 0 finishes, robot 1 reaches wp 0 and spends its budget on the unreachable wp 1, robot 2 has no waypoints,
    robot 3 spends it on its first; a call shorter than the budget leaves both going."""
    from tests.test_follow_cpu import _GoToGoal
    starts = np.array([[0.9, 0.9], [0.9, 0.9], [0.0, 0.0], [-2.0, -2.0]])
    wp = np.array([[[1.0, 1.0], [1.0, 0.5]], [[1.0, 1.0], FAR], [[0.0, 0.0], [0.0, 0.0]], [[2.5, 2.5], [0.0, 0.0]]])
    nw = [2, 2, 0, 2]
    B, T = 12, 40
    r = follow_waypoints(_GoToGoal(), "point", starts, wp, nw, max_steps=T, leg_steps=B, path_stride=1)
    assert np.array_equal(r["status"], [FINISHED, STALLED, NO_WAYPOINTS, STALLED])
    short = follow_waypoints(_GoToGoal(), "point", starts, wp, nw, max_steps=5, leg_steps=B)
    assert np.array_equal(short["status"], [GOING, GOING, NO_WAYPOINTS, GOING])
    assert np.array_equal(short["state"].leg_used, [4, 4, 0, 5]) and np.array_equal(short["steps"], [5, 5, 0, 5])
    s = r["state"]
    assert r["arrival"][1, 0] == 1 and r["arrival"][1, 1] == -1
    assert r["steps"][1] == 1 + B and s.leg_used[1] == B          # the arrival step starts the leg: B more steps, then idle
    assert np.all(r["path"][1 + B:, 1] == r["path"][1 + B, 1])      # a stalled robot stays put
    assert s.leg_used[0] == 0 and r["steps"][0] == r["arrival"][0, 1]
    assert r["steps"][2] == 0 and np.isnan(r["final_distance"][2])
    assert r["steps"][3] == B and s.leg_used[3] == B and r["reached"][3] == 0
    assert s.step0 == T
    # a stalled robot runs no step in the next call ...
    r2 = follow_waypoints(_GoToGoal(), "point", max_steps=10, leg_steps=B, state=s)
    assert r2["steps"][1] == 1 + B and r2["status"][1] == STALLED and r2["state"].step0 == T + 10
    # ... without a budget it goes on, and a larger budget gives it the difference
    r3 = follow_waypoints(_GoToGoal(), "point", max_steps=10, leg_steps=B + 4, state=s)
    assert r3["steps"][1] == 1 + B + 4 and r3["status"][1] == STALLED
    with pytest.raises(ValueError, match="leg_used"):
        follow_waypoints(_GoToGoal(), "point", max_steps=10, leg_steps=B - 1, state=s)


def test_replan_bookkeeping():
    st = FollowState(np.zeros((4, 2)), SQUARE[:2], hazards=True)
    st.robot[:, 0], st.robot[:, 1], st.robot[:, 2] = [1.5, 2.5, 3.5, 4.5], 9, [2, 1, 0, 1]
    st.arrival[:] = [[3, 9], [4, -1], [-1, -1], [2, -1]]
    st.leg_used[:] = [0, 5, 9, 7]
    st.state[:] = np.arange(24).reshape(4, 6)
    st.hazard[:, 0] = 2.0
    before = st.copy()
    st.replan([1, 3], [[0.5, 0.5], [0.2, 0.1], [0.0, 0.0]], n_waypoints=[3, 1])      # K grows from 2 to 3
    assert st.waypoints.shape == (4, 3, 2) and st.arrival.shape == (4, 3)
    assert np.array_equal(st.n_waypoints, [2, 3, 2, 1])
    assert np.array_equal(st.waypoints[1], np.array([[0.5, 0.5], [0.2, 0.1], [0.0, 0.0]], np.float32))
    assert np.array_equal(st.waypoints[3], np.array([[0.5, 0.5], [0, 0], [0, 0]], np.float32))   # past the count: zeroed
    assert np.array_equal(st.waypoints[[0, 2], :2], before.waypoints[[0, 2]]) and np.all(st.waypoints[[0, 2], 2] == 0)
    assert np.array_equal(st.arrival, [[3, 9, -1], [-1, -1, -1], [-1, -1, -1], [-1, -1, -1]])
    assert np.array_equal(st.robot[:, 2], [2, 0, 0, 0]) and np.array_equal(st.leg_used, [0, 0, 9, 0])
    for k in ("state", "hazard"):                                                  # everything else is carried
        assert np.array_equal(getattr(st, k), getattr(before, k), equal_nan=True), k
    assert np.array_equal(st.robot[:, :2], before.robot[:, :2]) and st.step0 == before.step0
    assert np.array_equal(before.arrival, [[3, 9], [4, -1], [-1, -1], [2, -1]])    # copy() is deep
    st.replan([], SQUARE)
    for bad in ([4], [-1], [1, 1], [0.5]):
        with pytest.raises(ValueError):
            st.replan(bad, SQUARE)
    with pytest.raises(ValueError):
        st.replan([0], [[np.nan, 0.0]])
    with pytest.raises(ValueError):
        st.replan([0], np.zeros((1, 2, 3)))


def test_follow_with_replanning_toy_planner():
    """Every robot's only waypoint is unreachable; the planner hands stalled robots a reachable one, once."""
    from tests.test_follow_cpu import _GoToGoal
    n = 6
    starts = np.random.default_rng(1).uniform(-0.5, 0.5, (n, 2))
    wp = np.broadcast_to(FAR, (n, 1, 2)).copy()
    wp[0, 0] = [1.0, 1.0]                            # robot 0 needs no help
    seen = []

    def planner(pos, status, reached):
        seen.append((pos.copy(), status.copy(), reached.copy()))
        return {i: [[-1.0, 1.0], [0.0, 0.0]] for i in np.nonzero(status == STALLED)[0]}

    r = follow_with_replanning(_GoToGoal(), "point", starts, wp, planner, horizon=50, rounds=6, leg_steps=40)
    assert np.all(r["status"] == FINISHED)
    assert np.array_equal(r["reached"], [1] + [2] * (n - 1))
    assert r["round_status"].shape[1] == n and len(seen) == len(r["round_status"]) - 1 + (len(r["round_status"]) < 6)
    assert np.array_equal(r["round_status"][0], [FINISHED] + [STALLED] * (n - 1))
    assert seen[0][0].shape == (n, 2) and np.all(seen[0][2][1:] == 0)
    assert np.all(r["arrival"][1:, 0] > 50)          # global steps: the new waypoints were reached in a later round
    assert np.all(r["steps"][1:] > 40)               # steps run are the run's
    none = follow_with_replanning(_GoToGoal(), "point", starts, wp, lambda *a: None, horizon=50, rounds=6, leg_steps=40)
    assert np.array_equal(none["status"], [FINISHED] + [STALLED] * (n - 1)) and np.all(none["steps"][1:] == 40)
    for kw in (dict(horizon=0, rounds=2), dict(horizon=5, rounds=0)):
        with pytest.raises(ValueError):
            follow_with_replanning(_GoToGoal(), "point", starts, wp, planner, **kw)


def test_run_arguments_are_checked():
    from mobrob_amd.envs.goal_rules import Hazards
    from tests.test_follow_cpu import _GoToGoal
    pol, z = _GoToGoal(), np.zeros((2, 2))
    good = follow_waypoints(pol, "point", z, SQUARE, max_steps=3)["state"]
    with pytest.raises(ValueError):
        follow_waypoints(pol, "point", z, SQUARE, max_steps=3, leg_steps=-1)
    with pytest.raises(ValueError):
        follow_waypoints(pol, "point", z, SQUARE, max_steps=3, state=good)          # start / waypoints beside a state
    with pytest.raises(ValueError):
        follow_waypoints(pol, "point", max_steps=3)                                   # neither
    with pytest.raises(TypeError):
        follow_waypoints(pol, "point", max_steps=3, state={"step0": 0})
    with pytest.raises(ValueError):
        follow_waypoints(pol, "point", max_steps=3, state=good, hazards=Hazards(np.zeros((1, 2)), 0.3))
    with pytest.raises(ValueError):
        follow_waypoints(pol, "doggo", max_steps=3, state=FollowState(np.zeros((2, 3)), np.zeros((1, 3))))   # doggo: P = 2

    def broken(**kw):
        s = good.copy()
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(s, k)[v[0]] = v[1]
            else:
                setattr(s, k, v)
        return s
    for s in (broken(step0=-1), broken(step0=2 ** 31 - 2), broken(state=((0, 4), np.nan)), broken(state=((1, 0), np.inf)),
              broken(robot=((0, 0), np.nan)), broken(robot=((1, 2), 5.0)), broken(robot=((1, 2), -1.0)),
              broken(leg_used=(0, 1)), broken(leg_used=(1, -1))):
        with pytest.raises(ValueError):
            follow_waypoints(pol, "point", max_steps=3, state=s)
    assert follow_waypoints(pol, "point", max_steps=3, state=good)["state"].step0 == 6
    assert good.step0 == 3                                                           # the given state is left as it was


def test_resume_struct_layout_is_the_c_compiler_s(tmp_path):
    from mobrob_amd import _lib
    names = [n for n, _ in _lib.FollowResume._fields_]
    assert names == ["step0", "leg_steps", "state", "leg_used", "status"]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "mobrob_ppo.h"\nint main(void) {\n'
            '  printf("%zu\\n", sizeof(mobrob_follow_resume_t));\n'
            + "".join(f'  printf("%zu\\n", offsetof(mobrob_follow_resume_t, {n}));\n' for n in names) + "  return 0;\n}\n")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(prog)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(_lib.FollowResume)
    assert out[1:] == [getattr(_lib.FollowResume, n).offset for n in names]
    assert "mobrob_ppo_follow_waypoints_resume" in _lib.SYMBOLS


def _load_script():
    spec = importlib.util.spec_from_file_location("follow_cli", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_chain_arguments():
    cli = _load_script()
    assert cli.check_chain(1000, None, 0) == [1000]
    assert cli.check_chain(1000, 50, 0) == [50] * 20
    assert cli.check_chain(120, 50, 7) == [50, 50, 20]
    assert cli.check_chain(30, 50, 0) == [30]
    for bad in ((0, None, 0), (100, 0, 0), (100, -5, 0), (100, 10, -1)):
        with pytest.raises(ValueError):
            cli.check_chain(*bad)


@pytest.mark.parametrize("extra", [["--horizon", "0"], ["--leg-steps", "-3"], ["--horizon", "x"]])
def test_cli_refuses_bad_chain_arguments_before_loading_anything(extra, tmp_path):
    np.save(tmp_path / "sq.npy", SQUARE)
    r = subprocess.run([sys.executable, SCRIPT, "--waypoints", str(tmp_path / "sq.npy")] + extra, cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 2 and "usage:" in r.stderr


def test_cli_host_chain_prints_what_the_single_call_prints(capsys):
    """--host with a scripted policy: the chained run's report lines are the single call's, character for character."""
    cli = _load_script()
    pol = _Scripted()
    cli.follow("point", "ppo", SQUARE, 6, max_steps=150, host=True, seed=3, policy=pol)
    single = capsys.readouterr().out
    cli.follow("point", "ppo", SQUARE, 6, max_steps=150, host=True, seed=3, policy=pol, horizon=40)
    chained = capsys.readouterr().out
    assert single == chained and single.startswith("success rate: ")
    cli.follow("point", "ppo", SQUARE, 6, max_steps=150, host=True, seed=3, policy=pol, horizon=40, leg_steps=30)
    assert "stalled rate: " in capsys.readouterr().out
