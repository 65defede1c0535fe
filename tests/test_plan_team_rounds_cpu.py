"""CPU: the rule of priority reordering rounds (goal_rules.grid_plan_team(order=), plan_team_next_order, grid_plan_team_rounds) and
the host path of GridPlanner(..., retries=).  Integers and bit patterns throughout: nothing here has a tolerance."""
import numpy as np
import pytest

from mobrob_amd.envs import goal_rules as R
from mobrob_amd.envs.goal_rules import grid_plan_team, grid_plan_team_rounds
from mobrob_amd.planning import GridPlanner
from tests.plan_scenes import EXTENT, INFLATE
from tests.plan_team_rounds_scenes import CORRIDOR_K, CORRIDOR_TABLE, CORRIDOR_TIME, ROUNDS_KEYS, corridor_case, hopeless_pair, permuted
from tests.plan_team_scenes import TEAM_KEYS, circling32, lattice_case, same_team, sealed_case, swap_case, teams

PER_ROBOT = ("waypoints", "n_waypoints", "count", "status", "cost", "waits", "leave", "arrive", "release", "fields", "field_goal_cell", "field_scene")


@pytest.fixture(scope="module")
def corridor():
    """the corridor's plans by the rule, computed once: {(reserve, retries): dict} and the plain team plan per reserve"""
    spec, walls, start, goal = corridor_case()
    plain = {r: grid_plan_team(spec, walls, None, start, goal, CORRIDOR_K, teams(4), r, **CORRIDOR_TIME) for r in (0, 1)}
    rounds = {(r, n): grid_plan_team_rounds(spec, walls, None, start, goal, CORRIDOR_K, teams(4), r, retries=n, **CORRIDOR_TIME)
              for r in (0, 1) for n in (0, 1, 2, 3)}
    return plain, rounds


@pytest.mark.parametrize("r", [0, 1])
def test_corridor_without_retries_is_todays_plan(corridor, r):
    plain, rounds = corridor
    got = rounds[r, 0]
    same_team(got, plain[r])
    assert got["walks"] == plain[r]["walks"]
    status, cost0, cost1 = CORRIDOR_TABLE[0, 1, 2, 3]
    assert got["status"].tolist() == status and got["cost"].tolist() == (cost0, cost1)[r]
    assert got["team_order"].tolist() == [[0, 1, 2, 3]] and got["team_order"].dtype == np.int32
    assert got["team_rounds"].tolist() == [1] and got["team_parked"].tolist() == [2] and got["team_parked_first"].tolist() == [2]


@pytest.mark.parametrize("r", [0, 1])
def test_corridor_one_retry_parks_one(corridor, r):
    got = corridor[1][r, 1]
    status, cost0, cost1 = CORRIDOR_TABLE[1, 2, 0, 3]
    assert got["team_order"].tolist() == [[1, 2, 0, 3]] and got["team_rounds"].tolist() == [2]
    assert got["team_parked"].tolist() == [1] and got["team_parked_first"].tolist() == [2]
    assert got["status"].tolist() == status and got["cost"].tolist() == (cost0, cost1)[r]
    assert got["team_clearance"][0] > r and got["team_crossings"][0] == 0


@pytest.mark.parametrize("retries", [2, 3])
@pytest.mark.parametrize("r", [0, 1])
def test_corridor_two_retries_park_nobody(corridor, r, retries):
    got = corridor[1][r, retries]
    status, cost0, cost1 = CORRIDOR_TABLE[2, 1, 0, 3]
    assert got["team_order"].tolist() == [[2, 1, 0, 3]] and got["team_rounds"].tolist() == [3]
    assert got["team_parked"].tolist() == [0] and got["team_parked_first"].tolist() == [2]
    assert got["status"].tolist() == status and got["cost"].tolist() == (cost0, cost1)[r]
    assert got["team_clearance"].tolist() == [r + 1] and got["team_clearance"][0] > r and got["team_crossings"].tolist() == [0]
    spec, walls, start, goal = corridor_case()
    ordered = grid_plan_team(spec, walls, None, start, goal, CORRIDOR_K, teams(4), r, order=[[2, 1, 0, 3]], **CORRIDOR_TIME)
    same_team(got, ordered)                                                   # the result is that round's ordered plan, bit for bit
    assert got["walks"] == ordered["walks"]


@pytest.fixture(scope="module")
def circling():
    """circling32's team plans by the rule, computed once per size: (plain, identity order, rounds at retries=3)"""
    spec, walls, hz, start, goal = circling32()
    out = {}
    for size in (2, 4, 16):
        args = (spec, walls, hz, start, goal, 4, teams(size), 1, 0, 10, 8)
        ident = np.tile(np.arange(size), (32 // size, 1))
        out[size] = (grid_plan_team(*args), grid_plan_team(*args, order=ident), grid_plan_team_rounds(*args, retries=3))
    return out


@pytest.mark.parametrize("size", [2, 4, 16])
def test_identity_order_is_the_team_plan(circling, size):
    plain, ident, _ = circling[size]
    same_team(ident, plain, TEAM_KEYS)
    assert ident["walks"] == plain["walks"]


@pytest.mark.parametrize("size", [2, 4, 16])
def test_an_order_is_the_team_plan_of_the_permuted_robots(size):
    spec, walls, hz, start, goal = circling32()
    order = np.stack([np.arange(size)[::-1] if g % 2 else np.roll(np.arange(size), 1) for g in range(32 // size)])   # reversed, or the last first
    assert np.any(order != np.arange(size))
    got = grid_plan_team(spec, walls, hz, start, goal, 4, teams(size), 1, 0, 10, 8, order=order)
    ref = grid_plan_team(spec, walls, hz, permuted(start, order, size), permuted(goal, order, size), 4, teams(size), 1, 0, 10, 8)
    rows = np.arange(32) // size * size + order.ravel()
    for k in PER_ROBOT:
        assert np.array_equal(got[k][rows].view(np.uint32), ref[k].view(np.uint32)), k
    for k in ("team_clearance", "team_crossings", "occupancy", "field_of"):
        assert np.array_equal(got[k], ref[k]), k
    assert [got["walks"][i] for i in rows] == ref["walks"]


@pytest.mark.parametrize("size", [2, 4, 16])
def test_rounds_never_park_more_than_index_order(circling, size):
    plain, _, got = circling[size]
    assert np.all(got["team_parked"] <= got["team_parked_first"])
    assert np.array_equal(got["team_parked_first"], R.plan_team_parked(plain["status"]).reshape(-1, size).sum(axis=1))
    assert np.array_equal(got["team_parked"], R.plan_team_parked(got["status"]).reshape(-1, size).sum(axis=1))
    assert np.all((got["team_rounds"] >= 1) & (got["team_rounds"] <= 4))
    assert np.array_equal(np.sort(got["team_order"], axis=1), np.tile(np.arange(size), (32 // size, 1)))
    spec, walls, hz, start, goal = circling32()
    ordered = grid_plan_team(spec, walls, hz, start, goal, 4, teams(size), 1, 0, 10, 8, order=got["team_order"])
    same_team(got, ordered)
    assert got["walks"] == ordered["walks"]
    print("size", size, "rounds", got["team_rounds"].tolist(), "parked first", got["team_parked_first"].tolist(), "parked", got["team_parked"].tolist())


@pytest.mark.parametrize("case,size", [(swap_case, 2), (lattice_case, 16)])
def test_a_plan_without_failures_takes_one_round(case, size):
    spec, start, goal = case()
    plain = grid_plan_team(spec, None, None, start, goal, 16, teams(size), 1, 0, 10, 48)
    got = grid_plan_team_rounds(spec, None, None, start, goal, 16, teams(size), 1, 0, 10, 48, retries=3)
    same_team(got, plain)
    assert got["walks"] == plain["walks"]
    assert got["team_rounds"].tolist() == [1] and got["team_order"].tolist() == [list(range(size))]
    assert got["team_parked"].tolist() == [0] and got["team_parked_first"].tolist() == [0]


def test_a_hopeless_pair_stops_after_both_orders():
    spec, start, goal = hopeless_pair()
    plain = grid_plan_team(spec, None, None, start, goal, 8, teams(2), 1, 0, 10, 48)
    got = grid_plan_team_rounds(spec, None, None, start, goal, 8, teams(2), 1, 0, 10, 48, retries=3)
    assert plain["status"].tolist() == [R.PLANNED, R.UNREACHABLE]
    same_team(got, plain)                                                     # a tie: the earliest round, round 0
    assert got["team_rounds"].tolist() == [2] and got["team_order"].tolist() == [[0, 1]]
    assert got["team_parked"].tolist() == [1] and got["team_parked_first"].tolist() == [1]
    other = grid_plan_team(spec, None, None, start, goal, 8, teams(2), 1, 0, 10, 48, order=[[1, 0]])
    assert other["status"].tolist() == [R.UNREACHABLE, R.PLANNED]


def test_parked_member_already_first_takes_one_round():
    spec, walls, start, goal = sealed_case()
    plain = grid_plan_team(spec, walls, None, start, goal, 8, teams(2), 1, 0, 10, 48)
    got = grid_plan_team_rounds(spec, walls, None, start, goal, 8, teams(2), 1, 0, 10, 48, retries=3)
    assert plain["status"].tolist() == [R.UNREACHABLE, R.PLANNED]
    same_team(got, plain)
    assert got["team_rounds"].tolist() == [1] and got["team_order"].tolist() == [[0, 1]] and got["team_parked"].tolist() == [1]


def test_next_order_keeps_relative_order():
    parked = np.zeros(6, bool)
    parked[[0, 4]] = True
    assert R.plan_team_next_order([3, 4, 1, 0, 5, 2], parked) == [4, 0, 3, 1, 5, 2]
    assert R.plan_team_next_order([4, 0, 3, 1, 5, 2], parked) == [4, 0, 3, 1, 5, 2]


def test_argument_errors_are_named():
    spec, start, goal = swap_case()
    args = (spec, None, None, start, goal, 8, teams(2), 1, 0, 10, 8)
    for bad in (-1, 9, True, 1.0, None):
        with pytest.raises(ValueError, match="retries"):
            grid_plan_team_rounds(*args, retries=bad)
    for bad in ([[0, 0]], [[0, 2]], [[0, 1], [1, 0]], [0, 1], [[0.0, 1.0]], [[True, False]]):
        with pytest.raises(ValueError, match="order"):
            grid_plan_team(*args, order=bad)
    with pytest.raises(ValueError, match="smooth"):
        grid_plan_team_rounds(*args, retries=1, smooth=True)
    smoothed = grid_plan_team_rounds(*args, retries=0, smooth=True)
    same_team(smoothed, grid_plan_team(*args, smooth=True))
    assert set(ROUNDS_KEYS) <= set(smoothed)


def test_planner_host_path_and_refusals():
    spec, walls, start, goal = corridor_case()
    kw = dict(walls=walls, cells=32, inflate=INFLATE, max_waypoints=CORRIDOR_K, extent=EXTENT, **CORRIDOR_TIME)
    planner = GridPlanner("point", teams=teams(4), reserve=1, retries=2, **kw)
    assert not planner.device and planner.retries == 2
    plan = planner.plan(start, goal)
    ref = grid_plan_team_rounds(spec, walls, None, start, goal, CORRIDOR_K, teams(4), 1, retries=2, want_fields=False, **CORRIDOR_TIME)
    same_team(plan, ref, ("waypoints", "n_waypoints", "count", "status", "cost", "waits", "leave", "arrive", "release", "team_clearance",
                          "team_crossings") + R.TEAM_ROUND_KEYS)
    assert plan["team_order"].tolist() == [[2, 1, 0, 3]] and plan["status"].tolist() == [0, 0, 0, 0]
    today = GridPlanner("point", teams=teams(4), reserve=1, **kw).plan(start, goal)
    assert today["status"].tolist() == [0, 1, 1, 0] and not set(R.TEAM_ROUND_KEYS) & set(today)
    rows = planner.callback(goal, horizon=20)(start.astype(np.float64), np.full(4, 2), np.zeros(4, bool))   # waypoints.STALLED == 2 is checked below
    from mobrob_amd.waypoints import STALLED
    assert STALLED == 2 and sorted(rows) == [0, 1, 2, 3]
    with pytest.raises(ValueError, match="retries= belongs to teams="):
        GridPlanner("point", retries=1, **{k: v for k, v in kw.items() if k not in CORRIDOR_TIME})
    with pytest.raises(ValueError, match="retries"):
        GridPlanner("point", teams=teams(4), retries=9, **kw)
    with pytest.raises(ValueError, match="retries > 0 with time_smooth"):
        GridPlanner("point", teams=teams(4), retries=1, time_smooth=True, **kw)
    with pytest.raises(ValueError, match="retries > 0 with time_smooth"):
        planner.plan(start, goal, time_smooth=True)
