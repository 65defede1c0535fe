"""CPU: goal assignment inside a team by the NumPy rule (goal_rules.grid_assign, plan_assign_match, plan_assign_team)
and the host path of GridPlanner(assign=).  The optimum is checked against ALL permutations up to size 8 and through the dual
certificate of the returned potentials at size 16; nothing here has a tolerance."""
import numpy as np
import pytest

from mobrob_amd.envs import goal_rules as R
from mobrob_amd.planning import GridPlanner
from tests import plan_assign_scenes as S
from tests.plan_scenes import EXTENT, INFLATE

NONE = R.PLAN_ASSIGN_NONE


@pytest.fixture(scope="module")
def ruled():
    """every scene by the rule, both objectives, computed once: {name: (scene, {objective: dict})}"""
    out = {}
    for name, make in S.SCENES.items():
        sc = make()
        out[name] = (sc, {obj: S.rule(sc, obj) for obj in S.OBJECTIVES})
    return out


def random_matrix(rng, size):
    """a seeded matrix with many ties (few distinct values) and NONEs"""
    C = rng.integers(0, 5, (size, size)).astype(np.int64) * 5 + rng.integers(0, 2, (size, size)) * 2
    C[rng.random((size, size)) < 0.2] = NONE
    return C


def key_of(C, col, objective):
    picked = C[np.arange(len(col)), col]
    return int(picked.sum()) if objective == "sum" else (int(picked.max()) << 32) + int(picked.sum())


@pytest.mark.parametrize("objective", S.OBJECTIVES)
@pytest.mark.parametrize("size", [2, 4, 8])
def test_optimum_against_all_permutations_on_random_matrices(size, objective):
    rng = np.random.default_rng(100 + size)
    for _ in range(40 if size < 8 else 6):
        C = random_matrix(rng, size)
        col, u, v, changed = R.plan_assign_team(C, objective)
        best, perms = S.optimum(C, objective)
        assert sorted(col.tolist()) == list(range(size)) and key_of(C, col, objective) == best
        assert changed == (col.tolist() != list(range(size)))
        if list(range(size)) in perms.tolist():
            assert not changed                                                   # identity first
        if objective == "sum":
            assert np.all(u[:, None] + v[None, :] <= C) and np.all(u + v[col] == C[np.arange(size), col])


@pytest.mark.parametrize("objective", S.OBJECTIVES)
@pytest.mark.parametrize("name", [n for n in S.SCENES if n != "sixteen"])
def test_scenes_against_all_permutations(ruled, name, objective):
    sc, outs = ruled[name]
    out, size = outs[objective], sc["size"]
    for t, C in enumerate(S.matrix(out)):
        col = out["assign"][t * size:(t + 1) * size] - t * size
        best, perms = S.optimum(C, objective)
        assert key_of(C, col, objective) == best
        assert bool(out["assign_changed"][t]) == (list(range(size)) not in perms.tolist())


@pytest.mark.parametrize("name", list(S.SCENES))
def test_scene_claims_outputs_and_certificate(ruled, name):
    sc, outs = ruled[name]
    sc["check"](outs)
    n, size = len(sc["goal"]), sc["size"]
    for objective, out in outs.items():
        S.certificate(out, objective)
        C = S.matrix(out)
        g = n // size
        assert out["assign"].dtype == np.int32 and np.array_equal(out["assign"] // size, np.arange(n) // size)     # inside the team
        assert np.array_equal(np.sort(out["assign"].reshape(g, size), axis=1), np.arange(n).reshape(g, size))
        assert out["goal"].dtype == np.float32 and np.array_equal(out["goal"], sc["goal"][out["assign"]])
        col = out["assign"].reshape(g, size) - (np.arange(g) * size)[:, None]
        picked = C[np.arange(g)[:, None], np.arange(size)[None, :], col]
        assert np.array_equal(out["assign_cost"], np.where(picked >= NONE, -1, picked).reshape(-1)) and out["assign_cost"].dtype == np.int32
        assert np.array_equal(out["assign_total"], picked.sum(axis=1)) and out["assign_total"].dtype == np.int64
        assert np.array_equal(out["assign_max"], picked.max(axis=1))
        ident = C[:, np.arange(size), np.arange(size)]
        assert np.array_equal(out["assign_identity_total"], ident.sum(axis=1)) and np.array_equal(out["assign_identity_max"], ident.max(axis=1))
        assert np.array_equal(out["assign_changed"], np.any(col != np.arange(size), axis=1)) and out["assign_changed"].dtype == bool
        assert np.all(out["assign_status"] == R.PLANNED)
        assert np.all(out["assign_total"] <= out["assign_identity_total"])
    assert np.all(outs["makespan"]["assign_max"] <= outs["sum"]["assign_max"])
    assert np.all(outs["sum"]["assign_total"] <= outs["makespan"]["assign_total"])


def test_matrix_is_the_field_at_the_start_cells(ruled):
    sc, outs = ruled["sixteen"]
    occ = R.grid_occupancy(sc["spec"], sc["walls"], None)
    scell, gcell = R.plan_assign_cells(sc["spec"], sc["start"], sc["goal"])
    m = outs["sum"]["assign_matrix"]
    for i, j in ((0, 3), (17, 30), (47, 32), (20, 16)):                             # (robot, mate whose goal)
        field = R.grid_field(occ[sc["walls"].scene[i]], gcell[j]).reshape(-1)
        assert m[i // 16, i % 16, j % 16] == field[scell[i]]


def test_size_16_against_scipy(ruled):
    opt = pytest.importorskip("scipy.optimize")
    sc, outs = ruled["sixteen"]
    for t, C in enumerate(S.matrix(outs["sum"])):
        r, c = opt.linear_sum_assignment(C)
        assert int(C[r, c].sum()) == int(outs["sum"]["assign_total"][t])


def test_team_of_one_is_the_identity():
    sc = S.crossed()
    out = R.grid_assign(sc["spec"], sc["walls"], None, sc["start"], sc["goal"], S.teams(1), "makespan")
    assert out["assign"].tolist() == [0, 1, 2, 3] and not out["assign_changed"].any() and out["assign_matrix"].shape == (4, 1, 1)
    assert np.array_equal(out["assign_cost"], out["assign_matrix"].reshape(-1))


def planner_kw(sc, **more):
    return dict(walls=sc["walls"], hazards=sc["hazards"], teams=S.teams(sc["size"]), reserve=1, cells=32, inflate=INFLATE, extent=EXTENT,
                max_waypoints=8, layer_steps=sc["time"].get("layer_steps", 10), layers=sc["time"].get("layers", 24), **more)


def same_dict(a, b, keys=None):
    assert keys is not None or sorted(a) == sorted(b)
    for k in (keys or a):
        x, y = a[k], b[k]
        if isinstance(x, R.Schedule):
            assert np.array_equal(x.release, y.release)
        elif isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), k
        else:
            assert x == y, k


@pytest.mark.parametrize("path", ["plain", "retries", "time_smooth"])
def test_host_planner_assigns_then_plans(ruled, path):
    sc, outs = ruled["crossed"]
    more = {"plain": {}, "retries": dict(retries=2), "time_smooth": dict(time_smooth=True)}[path]
    planner = GridPlanner("point", assign="sum", **planner_kw(sc, **more))
    assert not planner.device
    plan = planner.plan(sc["start"], sc["goal"])
    ref = outs["sum"]
    same_dict(plan, ref, R.ASSIGN_KEYS)
    same_dict(planner.assign(sc["start"], sc["goal"], want_matrix=True), ref, R.ASSIGN_KEYS + ("assign_matrix",))
    kw = dict(layer_steps=10, layers=24)
    if path == "retries":
        direct = R.grid_plan_team_rounds(sc["spec"], sc["walls"], None, sc["start"], ref["goal"], 8, S.teams(2), 1, retries=2, **kw)
    else:
        direct = R.grid_plan_team(sc["spec"], sc["walls"], None, sc["start"], ref["goal"], 8, S.teams(2), 1, smooth=path == "time_smooth", **kw)
    keys = ["waypoints", "n_waypoints", "count", "status", "cost", "waits", "leave", "arrive", "release", "team_clearance", "team_crossings",
            "field_of", "field_goal_cell", "field_scene"] + (list(R.TEAM_ROUND_KEYS) if path == "retries" else [])
    same_dict(plan, direct, keys)
    # and it is the plan of a planner WITHOUT assign= on the assigned goals, key for key
    plain = GridPlanner("point", **planner_kw(sc, **more)).plan(sc["start"], ref["goal"])
    same_dict({k: v for k, v in plan.items() if k not in R.ASSIGN_KEYS}, plain)


def test_crossed_plan_parks_nobody_and_costs_less(ruled):
    sc, _ = ruled["crossed"]
    kw = planner_kw(sc)
    given = GridPlanner("point", **kw).plan(sc["start"], sc["goal"])
    assigned = GridPlanner("point", assign="sum", **kw).plan(sc["start"], sc["goal"])
    assert not R.plan_team_parked(assigned["status"]).any()
    assert np.all(given["cost"] >= 0) and assigned["cost"].sum() < given["cost"].sum()
    assert np.array_equal(assigned["waypoints"][np.arange(4), assigned["n_waypoints"] - 1], assigned["goal"])


def test_assign_none_is_the_previous_plan(ruled):
    sc, _ = ruled["crossed"]
    kw = planner_kw(sc)
    direct = R.grid_plan_team(sc["spec"], sc["walls"], None, sc["start"], sc["goal"], 8, S.teams(2), 1, layer_steps=10, layers=24)
    for planner in (GridPlanner("point", **kw), GridPlanner("point", assign=None, **kw)):
        plan = planner.plan(sc["start"], sc["goal"])
        assert sorted(plan) == sorted(["waypoints", "n_waypoints", "count", "status", "cost", "field_of", "field_goal_cell", "field_scene",
                                       "fields_reused", "waits", "leave", "arrive", "release", "schedule", "team_clearance", "team_crossings",
                                       "cost_distance", "smoothed", "moves"])
        same_dict(plan, direct, ["waypoints", "n_waypoints", "count", "status", "cost", "waits", "leave", "arrive", "release", "team_clearance",
                                 "team_crossings"])


def test_grow_plans_the_same_assignment_and_the_callback_never_reassigns(ruled):
    sc, outs = ruled["crossed"]
    planner = GridPlanner("point", assign="sum", **dict(planner_kw(sc), max_waypoints=1))
    plan = planner.plan(sc["start"], sc["goal"], grow=True)
    same_dict(plan, outs["sum"], R.ASSIGN_KEYS)
    assert np.all(plan["status"] == R.PLANNED)
    from mobrob_amd.waypoints import STALLED
    cb = planner.callback(sc["goal"], horizon=10)                                   # the goals AS GIVEN: planned as given
    cb(sc["start"], np.full(4, STALLED), None)
    assert "assign" not in cb.last and planner.assign_objective == "sum"
    assert np.array_equal(cb.last["field_goal_cell"], R.plan_assign_cells(sc["spec"], sc["start"], sc["goal"])[1])


def test_refusals_are_named(ruled):
    sc, _ = ruled["crossed"]
    spec, walls, start, goal = sc["spec"], sc["walls"], sc["start"], sc["goal"]
    with pytest.raises(TypeError, match="Teams"):
        R.grid_assign(spec, walls, None, start, goal, 2)
    with pytest.raises(ValueError, match="objective"):
        R.grid_assign(spec, walls, None, start, goal, S.teams(2), "max")
    with pytest.raises(ValueError, match="objective"):
        R.grid_assign(spec, walls, None, start, goal, S.teams(2), None)
    with pytest.raises(ValueError, match="teams of 16"):
        R.grid_assign(spec, walls, None, start, goal, S.teams(16))
    bad = goal.copy()
    bad[1, 0] = np.nan
    with pytest.raises(ValueError, match="finite"):
        R.grid_assign(spec, walls, None, start, bad, S.teams(2))
    with pytest.raises(ValueError, match="finite"):
        R.grid_assign(spec, walls, None, np.where(bad != bad, np.inf, bad), goal, S.teams(2))
    with pytest.raises(ValueError, match="shapes"):
        R.grid_assign(spec, walls, None, start[:2], goal, S.teams(2))
    six = S.sixteen()
    with pytest.raises(ValueError, match="one scene"):
        R.grid_assign(spec, S.two_scenes(np.arange(48) % 2), None, six["start"], six["goal"], S.teams(16))
    mov = S.moving()
    for time in ({}, dict(layer_steps=3), dict(layers=4)):
        with pytest.raises(ValueError, match="layer_steps and layers"):
            R.grid_assign(spec, mov["walls"], mov["hazards"], mov["start"], mov["goal"], S.teams(4), **time)
    with pytest.raises(ValueError, match="square"):
        R.plan_assign_match(np.zeros((2, 3), np.int64))
    with pytest.raises(ValueError, match="assign= belongs to teams="):
        GridPlanner("point", assign="sum", cells=32, extent=EXTENT)
    with pytest.raises(ValueError, match="objective"):
        GridPlanner("point", assign="best", **planner_kw(sc))
    with pytest.raises(ValueError, match="no teams="):
        GridPlanner("point", cells=32, extent=EXTENT).assign(start, goal)


def test_follow_example_refuses_by_name():
    from examples.follow import build_parser, follow
    goals = np.zeros((2, 2))
    with pytest.raises(ValueError, match="--goals excludes"):
        follow("point", "ppo", None, 4, goal=[1.0, 1.0], goals=goals)
    with pytest.raises(ValueError, match="--assign needs"):
        follow("point", "ppo", None, 4, goals=goals, assign="sum")
    with pytest.raises(ValueError, match="--assign needs"):
        follow("point", "ppo", None, 4, goal=[1.0, 1.0], team_size=2, assign="sum")
    args = build_parser().parse_args(["--goals", "g.npy", "--assign", "makespan", "--team-size", "2"])
    assert (args.goals, args.assign) == ("g.npy", "makespan")
