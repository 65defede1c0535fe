"""CPU: waypoint following's host loop (mobrob_amd.waypoints, the statement of the semantics) with a NumPy go-to-goal policy,
its input checks, and the ctypes mirror of mobrob_follow_spec_t."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from mobrob_amd.envs.wrapper import get_env
from mobrob_amd.waypoints import follow_inputs, follow_waypoints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQUARE = np.array([[1.0, 1.0], [1.0, -1.0], [-1.0, -1.0], [-1.0, 1.0]])


class _GoToGoal:
    """predict(obs) = pinv(mix) . unit vector to the goal (obs[:P]): a command of speed `gain` towards the goal."""

    def __init__(self, env_name="point", gain=1.0):
        env = get_env(env_name)
        self.P = env.env.pos_dim
        self.A = np.linalg.pinv(env.env._mix) * gain
        self.calls = 0

    def predict(self, obs, deterministic=True):
        self.calls += 1
        return np.clip(self.A @ np.asarray(obs, np.float64)[:self.P], -1.0, 1.0), None


def test_host_loop_follows_a_square_in_order():
    starts = np.array([[0.0, 0.0], [0.5, -0.2], [-1.2, 0.3]])
    r = follow_waypoints(_GoToGoal(), "point", starts, SQUARE, max_steps=600, path_stride=1)
    assert r["persistent"] is None and r["trace"] is None
    assert np.array_equal(r["reached"], [4, 4, 4])
    arr = r["arrival"]
    assert np.all(arr > 0) and np.all(np.diff(arr, axis=1) > 0)          # strictly increasing, one waypoint per step at most
    assert np.array_equal(r["steps"], arr[:, -1])                          # finished robots stop at the last arrival
    assert np.all(r["final_distance"] < 0.3)
    path = r["path"]
    assert path.shape == (601, 3, 2)
    assert np.allclose(path[0], starts)
    for i in range(3):
        for k in range(4):                                                 # at its arrival the robot is inside the radius
            assert np.linalg.norm(path[arr[i, k], i] - SQUARE[k]) < 0.3
        assert np.all(path[arr[i, -1]:, i] == path[arr[i, -1], i])           # a finished robot repeats its last position
    assert np.all(np.isfinite(r["reward_sum"])) and np.all(r["reward_sum"] > 4 * 5.0)   # four reach bonuses plus progress


def test_host_loop_ragged_counts_and_zero_waypoints():
    starts = np.zeros((3, 2))
    wp = np.broadcast_to(SQUARE, (3, 4, 2)).copy()
    wp[0, 1:] = np.nan                                                      # slots past a robot's count are ignored
    pol = _GoToGoal()
    r = follow_waypoints(pol, "point", starts, wp, n_waypoints=[1, 0, 4], max_steps=500, path_stride=7)
    assert np.array_equal(r["reached"], [1, 0, 4])
    assert r["arrival"][0, 0] > 0 and np.all(r["arrival"][0, 1:] == -1)
    assert np.all(r["arrival"][1] == -1) and r["steps"][1] == 0 and r["reward_sum"][1] == 0.0
    assert np.isnan(r["final_distance"][1]) and np.all(r["path"][:, 1] == 0.0)
    assert r["steps"][0] == r["arrival"][0, 0] and r["steps"][2] == r["arrival"][2, 3]
    assert r["path"].shape == (500 // 7 + 1, 3, 2)
    assert pol.calls == r["steps"].sum()                                    # one predict per robot and step run


def test_host_loop_unreachable_waypoint_runs_max_steps():
    r = follow_waypoints(_GoToGoal(), get_env("point", time_limit=50), np.zeros((1, 2)), [[5.0, 5.0], [0.0, 0.0]], max_steps=120)
    assert r["reached"][0] == 0 and r["steps"][0] == 120 and np.all(r["arrival"] == -1)   # outside +-extent: never reached
    assert r["final_distance"][0] > 2.0


def test_a_start_inside_the_first_radius_counts_after_one_step():
    r = follow_waypoints(_GoToGoal(), "point", np.array([[1.0, 1.0]]), SQUARE[:2], max_steps=300)
    assert r["arrival"][0, 0] == 1


def test_zero_policy_reaches_nothing():
    class Zero:
        def predict(self, obs, deterministic=True):
            return np.zeros(2), None
    r = follow_waypoints(Zero(), "point", np.zeros((2, 2)), SQUARE, max_steps=50)
    assert np.all(r["reached"] == 0) and np.all(r["steps"] == 50)


@pytest.mark.parametrize("start, wp, nw", [
    (np.zeros(2), SQUARE, None),                                      # start not [n][P]
    (np.zeros((2, 3)), SQUARE, None),                                 # wrong pos_dim
    (np.zeros((2, 2)), np.zeros((3, 4, 2)), None),                    # robot count mismatch
    (np.zeros((2, 2)), np.zeros((2, 0, 2)), None),                    # K = 0
    (np.zeros((2, 2)), SQUARE, [1, 5]),                               # count > K
    (np.zeros((2, 2)), SQUARE, [-1, 2]),                              # negative count
    (np.zeros((2, 2)), SQUARE, [1.0, 2.0]),                           # non-integer counts
    (np.array([[0.0, np.nan], [0.0, 0.0]]), SQUARE, None),            # non-finite start
    (np.zeros((2, 2)), np.array([[np.inf, 0.0]]), None),              # non-finite waypoint
])
def test_bad_inputs_are_refused(start, wp, nw):
    with pytest.raises(ValueError):
        follow_waypoints(_GoToGoal(), "point", start, wp, nw, max_steps=10)


def test_bad_arguments_are_refused():
    with pytest.raises(ValueError):
        follow_waypoints(_GoToGoal(), "point", np.zeros((1, 2)), SQUARE, max_steps=0)
    with pytest.raises(ValueError):
        follow_waypoints(_GoToGoal(), "point", np.zeros((1, 2)), SQUARE, path_stride=-1)
    with pytest.raises(TypeError):
        follow_waypoints(_GoToGoal(), object(), np.zeros((1, 2)), SQUARE)
    with pytest.raises(ValueError, match="not found"):
        follow_waypoints(_GoToGoal(), "nosuchrobot", np.zeros((1, 2)), SQUARE)


def test_follow_inputs_broadcasts_and_zeroes_unused_slots():
    s, wp, nw = follow_inputs(np.ones((3, 2)), SQUARE, [4, 2, 0], pos_dim=2)
    assert s.dtype == np.float32 and wp.dtype == np.float32 and nw.dtype == np.int32
    assert wp.shape == (3, 4, 2) and np.array_equal(nw, [4, 2, 0])
    assert np.array_equal(wp[0], SQUARE) and np.all(wp[1, 2:] == 0) and np.all(wp[2] == 0)


def test_follow_spec_struct_size_and_offsets_are_the_c_compiler_s(tmp_path):
    """sizeof / offsetof of mobrob_follow_spec_t as gcc lays the header out == the ctypes mirror (every field, by name)."""
    from mobrob_amd import _lib
    names = [n for n, _ in _lib.FollowSpec._fields_]
    assert names == ["n_robots", "max_waypoints", "max_steps", "deterministic", "seed", "path_stride", "trace_robots",
                     "trace_steps"]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "mobrob_ppo.h"\nint main(void) {\n'
            '  printf("%zu\\n", sizeof(mobrob_follow_spec_t));\n'
            + "".join(f'  printf("%zu\\n", offsetof(mobrob_follow_spec_t, {n}));\n' for n in names) + "  return 0;\n}\n")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(prog)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(_lib.FollowSpec)
    assert out[1:] == [getattr(_lib.FollowSpec, n).offset for n in names]
    assert "mobrob_ppo_follow_waypoints" in _lib.SYMBOLS


def test_waypoints_module_never_imports_the_oracle():
    src = open(os.path.join(ROOT, "mobrob_amd", "waypoints.py")).read()
    assert "oracle" not in src
    assert "oracle" not in open(os.path.join(ROOT, "examples", "follow.py")).read()
