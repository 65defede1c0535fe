"""CPU: the team rule (goal_rules.Teams / team_cost / team_fold) and teams on the host loop of mobrob_amd.waypoints.

team_cost is float32 in the device's order; the reference here is a plain float64 double loop.  Cost tolerance: a distance
is a float32 sqrt of a float32 sum of two float32 products of float32 differences, 5 roundings of relative size 2^-24 on
quantities no larger than the arena's diagonal (< 8 in these tests), then up to 15 terms summed in float32 and one product with
the coefficient: |error| <= 15 terms x (5 + 15 + 1) roundings x 8 x 2^-24 < 2e-4, asserted as 2e-4."""
import numpy as np
import pytest

from mobrob_amd.envs import goal_rules as rules
from mobrob_amd.envs.goal_rules import TEAM_START, Teams, team_cost, team_fold
from mobrob_amd.envs.wrapper import get_env
from mobrob_amd.waypoints import FINISHED, FollowState, follow_waypoints, follow_with_replanning

COST_TOL = 2e-4


def _loop64(pos, stepped, sep, coef, indicator):
    """the rule as a float64 double loop over the float32 positions"""
    pos = np.asarray(pos, np.float32).astype(np.float64)
    G = len(pos)
    cost, clear, partner = np.zeros(G), np.full(G, np.inf), np.full(G, -1)
    for i in range(G):
        if not stepped[i]:
            continue
        for j in range(G):
            if j == i:
                continue
            d = np.hypot(*(pos[i] - pos[j]))
            if d <= sep:
                cost[i] += coef * (sep - d)
            if d - sep < clear[i]:
                clear[i], partner[i] = d - sep, j
        if indicator:
            cost[i] = float(cost[i] > 0)
    return cost, clear, partner


@pytest.mark.parametrize("G", rules.TEAM_SIZES)
def test_team_cost_against_a_float64_double_loop(G):
    rng = np.random.default_rng(G)
    sep, coef = float(np.float32(0.9)), float(np.float32(1.7))
    charged = free = 0
    for trial in range(40):
        pos = rng.uniform(-2.5, 2.5, (G, 2)).astype(np.float32)
        stepped = rng.random(G) < 0.8
        want_c, want_cl, want_p = _loop64(pos, stepped, sep, coef, False)
        cost, clear, partner = team_cost(pos, stepped, sep, coef)
        assert cost.dtype == np.float32 and clear.dtype == np.float32
        assert np.all(np.abs(cost - want_c) <= COST_TOL), (trial, cost, want_c)
        ind = team_cost(pos, stepped, sep, coef, True)[0]
        for i in range(G):
            if not stepped[i] or G == 1:
                assert cost[i] == 0 and np.isposinf(clear[i]) and partner[i] == -1
                continue
            d = np.sort(np.hypot(*(pos[i].astype(np.float64) - np.delete(pos, i, 0).astype(np.float64)).T))
            if np.min(np.abs(d - sep)) > 1e-5:                 # no mate within rounding of the boundary: the conflict set is exact
                assert (cost[i] > 0) == (want_c[i] > 0) and ind[i] == float(want_c[i] > 0)
            if len(d) < 2 or d[1] - d[0] > 1e-5:               # no two clearances within rounding of a tie: the partner is exact
                assert partner[i] == want_p[i]
                assert abs(clear[i] - want_cl[i]) <= 8 * 2.0 ** -24 * 8
            charged, free = charged + (cost[i] > 0), free + (cost[i] == 0)
    if G > 1:
        assert charged > 0 and free > 0


def test_a_mate_exactly_on_the_boundary_costs_nothing():
    cost, clear, partner = team_cost([[0.0, 0.0], [0.5, 0.0]], [True, True], 0.5, 3.0)
    assert np.array_equal(cost, [0, 0]) and np.array_equal(clear, [0, 0]) and np.array_equal(partner, [1, 0])
    assert np.array_equal(team_cost([[0.0, 0.0], [0.5, 0.0]], [True, True], 0.5, 3.0, True)[0], [0, 0])     # not a conflict step
    rec = team_fold(np.tile(TEAM_START, (2, 1)), [[[0.0, 0.0], [0.5, 0.0]]], [[True, True]], Teams(2, 0.5, 3.0))
    assert np.array_equal(rec, [[0, 0, -1, 0, 1], [0, 0, -1, 0, 0]])
    inside = team_cost([[0.0, 0.0], [0.25, 0.0]], [True, True], 0.5, 3.0)
    assert np.array_equal(inside[0], [0.75, 0.75]) and np.array_equal(inside[1], [-0.25, -0.25])


def test_equal_clearances_go_to_the_lowest_index():
    # member 1 sits between members 0 and 2, and 3 is as far again: for 1 the mates 0, 2 (and, on a cross, 3) tie
    pos = [[-1.0, 0.0], [0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]
    cost, clear, partner = team_cost(pos, [True] * 4, 0.25)
    assert partner[1] == 0 and clear[1] == 0.75
    # the tie crosses quarters (mates 0, 2, 3 are in quarters 0, 2, 3) and, in a team of 8, sits inside one (mates 0 and 4)
    pos8 = [[1.0, 0.0], [9.0, 9.0], [9.0, -9.0], [-9.0, 9.0], [-1.0, 0.0], [0.0, 0.0], [-9.0, -9.0], [9.0, 0.0]]
    assert team_cost(pos8, [True] * 8, 0.25)[2][5] == 0
    rev = pos8[::-1]                                            # member 2 is now the centre, its tied mates are 3 and 7
    assert team_cost(rev, [True] * 8, 0.25)[2][2] == 3


def test_two_teams_on_top_of_each_other_are_blind_to_each_other():
    team = np.array([[0.0, 0.0], [2.0, 0.0]])
    pos = np.concatenate([team, team])[None]                    # robots 0 and 2, 1 and 3 coincide
    rec = team_fold(np.tile(TEAM_START, (4, 1)), pos, np.ones((1, 4), bool), Teams(2, 0.5))
    assert np.array_equal(rec[:, 0], [0, 0, 0, 0]) and np.array_equal(rec[:, 3], [1.5] * 4)
    assert np.array_equal(rec[:, 4], [1, 0, 3, 2])              # partners are global indices inside the own team
    one = team_fold(np.tile(TEAM_START, (4, 1)), pos, np.ones((1, 4), bool), Teams(4, 0.5))
    assert np.all(one[:, 0] == 0.5) and np.array_equal(one[:, 4], [2, 3, 0, 1])


def test_a_team_of_one():
    cost, clear, partner = team_cost([[0.3, 0.3]], [True], 5.0)
    assert cost[0] == 0 and np.isposinf(clear[0]) and partner[0] == -1
    rec = team_fold(np.tile(TEAM_START, (3, 1)), np.zeros((2, 3, 2)), [[True, True, False]] * 2, Teams(1, 5.0))
    assert np.array_equal(rec[:2], [[0, 0, -1, np.inf, -1]] * 2) and np.array_equal(rec[2], TEAM_START, equal_nan=True)


def test_fold_keeps_the_first_conflict_and_the_first_closest_partner():
    pos = np.zeros((4, 2, 2))
    pos[:, 1, 0] = [2.0, 0.5, 0.5, 2.0]                         # apart, close, as close again, apart
    rec = team_fold(np.tile(TEAM_START, (2, 1)), pos, np.ones((4, 2), bool), Teams(2, 1.0, 2.0), step0=10)
    assert np.array_equal(rec, [[2.0, 2, 12, -0.5, 1], [2.0, 2, 12, -0.5, 0]])
    again = team_fold(rec, pos[:1], [[True, False]], Teams(2, 1.0, 2.0), step0=14)      # robot 1 parked: nothing accounted for it
    assert np.array_equal(again, rec)


class _GoToGoal:
    """predict = the command that heads for the goal at full speed, whatever the noise"""

    def __init__(self, env_name="point"):
        env = get_env(env_name)
        self.P = env.env.pos_dim
        self.A = np.linalg.pinv(env.env._mix)

    def predict(self, obs, deterministic=True):
        v = np.asarray(obs, np.float64)[:self.P]
        return np.clip(self.A @ (v / max(np.linalg.norm(v), 1e-9)), -1.0, 1.0), None


def _crossing():
    """Team 0: robot 0 is parked on the origin (no waypoints), robot 1 drives through it.  Team 1: the same job shifted by
    (0, 1.5) with a mate that also moves, well clear of team 0's separation."""
    start = np.array([[0.0, 0.0], [-1.0, 0.05], [-1.0, 1.5], [1.0, 1.55]])
    wp = np.array([[[0.0, 0.0]], [[1.0, 0.05]], [[1.0, 1.5]], [[-1.0, 1.55]]])
    return start, wp, np.array([0, 1, 1, 1])


def test_a_parked_mate_charges_the_passing_robot_and_not_itself():
    start, wp, nw = _crossing()
    r = follow_waypoints(_GoToGoal(), "point", start, wp, nw, max_steps=60, seed=1, teams=Teams(2, 0.4, 2.0))
    assert r["steps"][0] == 0 and r["conflict_steps"][0] == 0 and r["team_cost_sum"][0] == 0
    assert np.isnan(r["min_team_clearance"][0]) and r["closest_partner"][0] == -1 and r["first_conflict"][0] == -1
    assert r["conflict_steps"][1] > 0 and r["team_cost_sum"][1] > 0 and r["closest_partner"][1] == 0
    assert r["first_conflict"][1] > 1 and -0.4 <= r["min_team_clearance"][1] < -0.3          # it passes 0.05 from the parked mate
    # both move in team 1: both are charged on the same steps while both move, and each names the other
    assert r["conflict_steps"][2] > 0 and r["first_conflict"][2] == r["first_conflict"][3]
    assert np.array_equal(r["closest_partner"][2:], [3, 2])
    assert np.array_equal(r["state"].team[:, 0], r["team_cost_sum"]) and r["status"][1] == FINISHED
    # nothing else changes
    plain = follow_waypoints(_GoToGoal(), "point", start, wp, nw, max_steps=60, seed=1)
    for k in plain:
        if k not in ("state", "trace", "persistent"):
            assert np.array_equal(plain[k], r[k], equal_nan=True), k
    assert np.array_equal(plain["state"].state, r["state"].state)


@pytest.mark.parametrize("split", [(25, 35), (1, 59), (20, 20, 20)])
def test_a_split_run_carries_the_team_record(split):
    start, wp, nw = _crossing()
    teams, pol = Teams(2, 0.4, 2.0), _GoToGoal()
    one = follow_waypoints(pol, "point", start, wp, nw, max_steps=60, seed=1, teams=teams)
    r = None
    for i, steps in enumerate(split):
        r = follow_waypoints(pol, "point", start if i == 0 else None, wp if i == 0 else None, nw if i == 0 else None,
                             max_steps=steps, seed=1, teams=teams, state=None if i == 0 else r["state"])
    assert np.array_equal(one["state"].team, r["state"].team, equal_nan=True)
    for k in ("team_cost_sum", "conflict_steps", "first_conflict", "min_team_clearance", "closest_partner", "arrival", "steps"):
        assert np.array_equal(one[k], r[k], equal_nan=True), k
    assert np.any(one["conflict_steps"] > 0)


def test_replan_and_copy_keep_the_team_record_and_the_loop_takes_teams():
    start, wp, nw = _crossing()
    teams, pol = Teams(2, 0.4, 2.0), _GoToGoal()
    r = follow_waypoints(pol, "point", start, wp, nw, max_steps=30, seed=1, teams=teams)
    st = r["state"]
    kept = st.team.copy()
    assert np.any(kept[:, 1] > 0)
    assert np.array_equal(st.copy().team, kept, equal_nan=True) and st.copy().team is not st.team
    st.replan([1], np.array([[-1.0, 0.05]]))
    assert np.array_equal(st.team, kept, equal_nan=True)
    fresh = FollowState(start, wp, nw, teams=True)
    assert np.array_equal(fresh.team, np.tile(TEAM_START, (4, 1)), equal_nan=True) and FollowState(start, wp, nw).team is None
    calls = []
    out = follow_with_replanning(pol, "point", start, wp, lambda pos, status, reached: calls.append(pos.shape) or {},
                                 horizon=30, rounds=2, n_waypoints=nw, seed=1, teams=teams)
    one = follow_waypoints(pol, "point", start, wp, nw, max_steps=60, seed=1, teams=teams)
    assert calls == [(4, 2)] and np.array_equal(out["state"].team, one["state"].team, equal_nan=True)


def test_refusals():
    for bad in (0, 3, 5, 32, -2, 2.0, True):
        with pytest.raises(ValueError):
            Teams(bad, 0.5)
    for sep in (-0.1, np.inf, np.nan):
        with pytest.raises(ValueError):
            Teams(2, sep)
    for cost in (-1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            Teams(2, 0.5, cost)
    with pytest.raises(ValueError):
        Teams(4, 0.5).check_robots(6)
    Teams(4, 0.5).check_robots(8)
    with pytest.raises(ValueError):
        team_cost(np.zeros((2, 3)), [True, True], 0.5)
    with pytest.raises(ValueError):
        team_fold(np.zeros((3, 5)), np.zeros((1, 3, 2)), np.ones((1, 3), bool), Teams(2, 0.5))
    start, wp, nw = _crossing()
    pol = _GoToGoal()
    with pytest.raises(ValueError):                             # 4 robots do not split into teams of 8
        follow_waypoints(pol, "point", start, wp, nw, max_steps=5, teams=Teams(8, 0.5))
    with pytest.raises(TypeError):
        follow_waypoints(pol, "point", start, wp, nw, max_steps=5, teams=(2, 0.5))
    plain = follow_waypoints(pol, "point", start, wp, nw, max_steps=5)
    with pytest.raises(ValueError):                             # a run has teams in every call or in none
        follow_waypoints(pol, "point", max_steps=5, state=plain["state"], teams=Teams(2, 0.5))
    team = follow_waypoints(pol, "point", start, wp, nw, max_steps=5, teams=Teams(2, 0.5))
    with pytest.raises(ValueError):
        follow_waypoints(pol, "point", max_steps=5, state=team["state"])
