"""CPU: the hazard cost rule (goal_rules.hazard_cost) against the reference's own Engine.cost executed on recorded cases
(tests/golden/hazard_cases.npz, made by tests/golden/make_hazard_fixture.py), EnvWrapper.set_hazards, the host waypoint loop's
hazard accounting against a hand computation, the Python-side checks and the ctypes mirror of mobrob_hazards_t."""
import ctypes
import os

import numpy as np
import pytest

from mobrob_amd.envs import goal_rules as rules
from mobrob_amd.envs.wrapper import get_env
from mobrob_amd.waypoints import follow_waypoints

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hazard_cases.npz")


def _cases():
    z = np.load(GOLDEN)
    for i in range(len(z["pos"])):
        m = int(z["n_hazards"][i])
        rows = np.concatenate([z["hazards"][i, :m], np.full((m, 1), z["size"][i])], axis=1).astype(np.float64)
        yield (i, z["pos"][i].astype(np.float64), rows, float(z["coef"][i]), float(z["cost_shaped"][i]),
               float(z["cost_indicator"][i]), bool(z["boundary"][i]))


def test_fixture_covers_the_issue_cases():
    z = np.load(GOLDEN)
    assert z["boundary"].sum() >= 3 and (z["n_hazards"] == 0).any() and (z["pos"][:, 2] != 0).any()
    assert (z["cost_shaped"] > 0).sum() >= 5 and ((z["cost_shaped"] == 0) & (z["n_hazards"] > 0)).any()
    assert (z["n_hazards"] > 1).any()


def test_hazard_cost_matches_reference_cases():
    for i, pos, rows, coef, shaped, ind, boundary in _cases():
        c, clear = rules.hazard_cost(pos, rows, coef, indicator=False)
        assert abs(c - shaped) <= 1e-12, (i, c, shaped)
        ci, clear_i = rules.hazard_cost(pos, rows, coef, indicator=True)
        assert ci == ind, (i, ci, ind)
        assert clear == clear_i
        if boundary:
            assert c == 0.0 and ci == 0.0, i
        if len(rows) == 0:
            assert clear == np.inf
        else:
            d = np.hypot(pos[0] - rows[:, 0], pos[1] - rows[:, 1])
            assert clear == np.min(d - rows[:, 2])


def test_hazard_cost_batched_matches_rows():
    cases = list(_cases())
    m = max(len(c[2]) for c in cases)
    for ind in (False, True):
        for i, pos, rows, coef, shaped, indc, _ in cases:
            if len(rows) == 0 or coef != 1.0:
                continue
            batch = np.stack([pos, pos + 0.0])
            c, _ = rules.hazard_cost(batch, rows, coef, ind)
            assert c.shape == (2,) and c[0] == c[1] == (indc if ind else rules.hazard_cost(pos, rows, coef, ind)[0])
    assert m >= 1


def test_envwrapper_info_costs():
    env = get_env("point")
    env.seed(3)
    env.reset()
    a = np.array([0.4, -0.3])
    _, _, _, _, info0 = env.step(a)
    assert "cost" not in info0 and "cost_hazards" not in info0           # without hazards: info as before
    for i, pos, rows, coef, shaped, ind, _ in _cases():
        for indicator, want in ((False, shaped), (True, ind)):
            env = get_env("drone" if pos[2] != 0 else "point")
            env.reset()
            env.set_hazards(rows[:, :2], rows[:, 2] if len(rows) else 0.3, coef, indicator)
            env.set_pos(pos)
            env.env.step = lambda act, e=env.env: (e.obs(), 0.0, False, False, {})   # hold the robot on the case's position
            _, _, _, _, info = env.step(np.zeros(env.action_space.shape))
            assert abs(info["cost_hazards"] - want) <= 1e-12 and info["cost"] == info["cost_hazards"], (i, info, want)
    env.set_hazards(None)
    _, _, _, _, info = env.step(np.zeros(env.action_space.shape))
    assert "cost" not in info


class _Straight:
    """predict = the action whose command is the constant velocity (g, 0): a straight line along +x."""

    def __init__(self, g):
        env = get_env("point")
        self.a = np.linalg.pinv(env.env._mix) @ np.array([g, 0.0])

    def predict(self, obs, deterministic=True):
        return self.a.copy(), None


def test_host_follow_hazard_hand_computation():
    # KinematicSim: vel_t = 0.8 vel_{t-1} + 0.2 u, pos_t = pos_{t-1} + dt vel_t, so x_t = x_0 + dt g sum_{k<=t} (1 - 0.8^k)
    g, dt, x0, T = 1.0, 0.05, -1.5, 80
    hx, r, c = 0.0, 0.3125, 2.0                                              # float32-exact: Hazards keeps float32
    x = x0 + dt * g * np.cumsum(1.0 - 0.8 ** np.arange(1, T + 1))
    d = np.abs(x - hx)
    assert np.min(np.abs(d - r)) > 1e-6                                      # no step on the boundary
    inside = d <= r
    want_first = int(np.argmax(inside)) + 1
    want_count = int(inside.sum())
    want_sum = float(np.sum(np.where(inside, c * (r - d), 0.0)))
    assert 0 < want_count < T
    hz = rules.Hazards([[hx, 0.0]], size=r, cost=c, indicator=False)
    res = follow_waypoints(_Straight(g), "point", [[x0, 0.0]], [[2.9, 0.0]], max_steps=T, hazards=hz)
    assert res["steps"][0] == T and res["reached"][0] == 0
    assert res["first_violation"][0] == want_first
    assert res["violation_steps"][0] == want_count
    assert abs(res["cost_sum"][0] - want_sum) <= 1e-9
    assert abs(res["min_clearance"][0] - np.min(d - r)) <= 1e-9
    hz_i = rules.Hazards([[hx, 0.0]], size=r, cost=c, indicator=True)
    res_i = follow_waypoints(_Straight(g), "point", [[x0, 0.0]], [[2.9, 0.0]], max_steps=T, hazards=hz_i)
    assert res_i["cost_sum"][0] == want_count and res_i["first_violation"][0] == want_first
    plain = follow_waypoints(_Straight(g), "point", [[x0, 0.0]], [[2.9, 0.0]], max_steps=T)
    assert "cost_sum" not in plain
    for k in ("arrival", "steps", "reward_sum", "final_distance"):
        assert np.array_equal(plain[k], res[k], equal_nan=True)


def test_host_follow_empty_scene_and_idle_robot():
    hz = rules.Hazards(np.zeros((0, 2)))
    res = follow_waypoints(_Straight(1.0), "point", [[0.0, 0.0], [1.0, 1.0]], [[[2.9, 0.0]], [[0.0, 0.0]]], n_waypoints=[1, 0],
                           max_steps=5, hazards=hz)
    assert res["cost_sum"].tolist() == [0.0, 0.0] and res["first_violation"].tolist() == [-1, -1]
    assert res["min_clearance"][0] == np.inf and np.isnan(res["min_clearance"][1])


@pytest.mark.parametrize("kwargs", [
    dict(locations=[[0.0, 0.0, 0.0]]),                                        # not [M, 2]
    dict(locations=np.zeros((1, 1025, 2))),                                   # M > 1024
    dict(locations=[[np.nan, 0.0]]),                                          # non-finite coordinate
    dict(locations=[[0.0, 0.0]], size=np.inf),                                # non-finite radius
    dict(locations=[[0.0, 0.0]], size=-0.1),                                  # negative radius
    dict(locations=[[0.0, 0.0], [1.0, 1.0]], size=[0.3, 0.3, 0.3]),           # size of the wrong length
    dict(locations=[[0.0, 0.0]], cost=-1.0),                                  # negative cost
    dict(locations=[[0.0, 0.0]], cost=np.nan),
    dict(locations=[[0.0, 0.0]], counts=[2]),                                 # count > M
    dict(locations=[[0.0, 0.0]], counts=[-1]),
    dict(locations=np.zeros((2, 3, 2))),                                      # S > 1 without scene
    dict(locations=np.zeros((2, 3, 2)), scene=[0, 2]),                        # scene out of range
    dict(locations=np.zeros((2, 3, 2)), scene=[0.5, 1.0]),                    # scene not integers
    dict(locations=np.zeros((0, 3, 2))),                                      # no scene at all
])
def test_hazards_validation(kwargs):
    with pytest.raises(ValueError):
        rules.Hazards(**kwargs)


def test_hazards_scene_length_checked():
    hz = rules.Hazards(np.zeros((2, 3, 2)), scene=[0, 1, 1])
    with pytest.raises(ValueError):
        hz.check_robots(4)
    hz.check_robots(3)
    with pytest.raises(ValueError):
        follow_waypoints(_Straight(1.0), "point", np.zeros((2, 2)), [[1.0, 0.0]], max_steps=3, hazards=hz)


def test_hazards_struct_mirror():
    from mobrob_amd._lib import HazardsC
    assert ctypes.sizeof(HazardsC) == 40
    offs = {n: getattr(HazardsC, n).offset for n, _ in HazardsC._fields_}
    assert offs == {"n_scenes": 0, "max_hazards": 4, "hazards": 8, "n_hazards": 16, "scene": 24, "cost": 32, "indicator": 36}
