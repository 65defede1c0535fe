"""GPU: goal assignment inside a team on the device (mobrob_ppo_plan_assign: the base map, k_plan_assign_cost, k_plan_assign) against
the NumPy rule (goal_rules.grid_assign), BIT FOR BIT: every output array, the cost matrix and the potentials included -- the wave
runs goal_rules.plan_assign_match's scans in the rule's order, so (u, v) are the rule's own integers.  Nothing here has
a tolerance."""
import numpy as np
import pytest

from mobrob_amd.envs import goal_rules as R
from mobrob_amd.planning import GridPlanner
from tests import plan_assign_scenes as S
from tests.plan_scenes import EXTENT, INFLATE
from tests.util import _engine, _env, _snapshot

pytestmark = pytest.mark.gpu
KW = dict(pi=(64, 64), vf=(64, 64))


@pytest.fixture(scope="module")
def engine():
    e, _ = _engine("point", KW)
    yield e
    e.close()


def device(engine, sc, objective, **more):
    return engine.plan_assign(sc["spec"], sc["walls"], sc["hazards"], teams=S.teams(sc["size"]), start=sc["start"], goal=sc["goal"],
                              objective=objective, want_matrix=True, **sc["time"], **more)


@pytest.mark.parametrize("name", list(S.SCENES))
def test_scene_both_objectives(engine, name):
    sc = S.SCENES[name]()
    outs = {}
    for objective in S.OBJECTIVES:
        dev = outs[objective] = device(engine, sc, objective)
        S.same_assign(dev, S.rule(sc, objective))
        S.certificate(dev, objective)
        assert np.all(dev["sweeps"] >= 1) and np.all(dev["assign_status"] == R.PLANNED)
    sc["check"](outs)


@pytest.mark.parametrize("n_teams", [1, 33])
def test_team_counts(engine, n_teams):
    """one team, and 33 teams of 4: the rule's assignment of `walled`, shifted a cell per team"""
    sc = S.walled()
    shift = (np.arange(n_teams, dtype=np.float32) % 3 * np.float32(-0.125)).repeat(4)[:, None] * np.array([0, 1], np.float32)
    start, goal = np.tile(sc["start"], (n_teams, 1)) + shift, np.tile(sc["goal"], (n_teams, 1)) + shift
    dev = engine.plan_assign(sc["spec"], sc["walls"], None, teams=S.teams(4), start=start, goal=goal, want_matrix=True)
    ref = R.grid_assign(sc["spec"], sc["walls"], None, start, goal, S.teams(4))
    S.same_assign(dev, ref)
    assert dev["assign_changed"].all() and len(dev["assign_total"]) == n_teams


@pytest.mark.parametrize("path", ["retries", "time_smooth"])
def test_planner_on_the_device_against_the_host_planner(engine, path):
    sc = S.crossed()
    more = dict(retries=2) if path == "retries" else dict(time_smooth=True)
    kw = dict(walls=sc["walls"], teams=S.teams(2), reserve=1, cells=32, inflate=INFLATE, extent=EXTENT, max_waypoints=8, layer_steps=10,
              layers=24, assign="makespan", **more)
    dev_planner, host_planner = GridPlanner(_env("point", 4), engine=engine, **kw), GridPlanner("point", **kw)
    assert dev_planner.device and not host_planner.device
    dev, host = dev_planner.plan(sc["start"], sc["goal"]), host_planner.plan(sc["start"], sc["goal"])
    keys = ("waypoints", "n_waypoints", "count", "status", "cost", "waits", "leave", "arrive", "release", "team_clearance", "team_crossings",
            "cost_distance") + R.ASSIGN_KEYS + (R.TEAM_ROUND_KEYS if path == "retries" else ("moves",))
    for k in keys:
        assert dev[k].dtype == host[k].dtype and np.array_equal(dev[k], host[k], equal_nan=dev[k].dtype.kind == "f"), k
    assert dev["assign"].tolist() == [1, 0, 2, 3] and not R.plan_team_parked(dev["status"]).any()
    assert np.array_equal(dev["schedule"].release, host["schedule"].release)
    S.same_assign(dev_planner.assign(sc["start"], sc["goal"], want_matrix=True), S.rule(sc, "makespan"))


def test_training_untouched(engine):
    sc = S.sixteen()
    env_a, env_b = _env("point", 16, tl=40), _env("point", 16, tl=40)
    ea, _ = _engine("point", KW, seed=7)
    eb, _ = _engine("point", KW, seed=7)
    env_a.collect(ea)
    env_b.collect(eb)
    before = _snapshot(eb, stats=False)
    got = device(eb, sc, "makespan")
    sa, sb = _snapshot(ea, stats=False), _snapshot(eb, stats=False)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]) and np.array_equal(before[k], sb[k]), k
    ea.train()
    eb.train()
    assert np.array_equal(ea.get_flat_params(), eb.get_flat_params())
    assert got["assign_changed"].all()
    ea.close()
    eb.close()


def test_engine_refusals_are_named(engine):
    sc = S.crossed()
    kw = dict(teams=S.teams(2), start=sc["start"], goal=sc["goal"])
    with pytest.raises(ValueError, match="objective"):
        engine.plan_assign(sc["spec"], sc["walls"], None, objective="max", **kw)
    with pytest.raises(TypeError, match="Teams"):
        engine.plan_assign(sc["spec"], sc["walls"], None, **dict(kw, teams=2))
    with pytest.raises(ValueError, match="finite"):
        engine.plan_assign(sc["spec"], sc["walls"], None, **dict(kw, goal=sc["goal"] * np.float32(np.inf)))
    mov = S.moving()
    with pytest.raises(ValueError, match="layer_steps and layers"):
        engine.plan_assign(mov["spec"], mov["walls"], mov["hazards"], teams=S.teams(4), start=mov["start"], goal=mov["goal"])
    six = S.sixteen()
    with pytest.raises(ValueError, match="one scene"):
        engine.plan_assign(six["spec"], S.two_scenes(np.arange(48) % 2), None, teams=S.teams(16), start=six["start"], goal=six["goal"])
