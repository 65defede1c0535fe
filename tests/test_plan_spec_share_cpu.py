"""CPU: a team shares the stations of a specification (goal_rules.spec_plan_best, spec_plan_share, spec_plan with share= and
objective=, spec_team_result).  The allotment is held to an independent brute force over every assignment of stations to members and
every visit order; share=1 to the plan without share=, bit for bit."""
import itertools

import numpy as np
import pytest

from mobrob_amd.envs import goal_rules as R
from tests.plan_spec_scenes import random_scene, symmetric_scene

NONE, INF = R.PLAN_ASSIGN_NONE, R.PLAN_TOUR_INF
KEYS = R.SPEC_PLAN_KEYS + R.SPEC_REPLAN_KEYS


def costs(seed, n, M, hard=False):
    """random legs and ticks for n robots -> dict(d0, D, E, e0, open_c, close_c, dwell_c, t0); `hard`: deadlines that bite, legs
    without a path"""
    rng = np.random.default_rng(seed)
    d0, D = rng.integers(5, 90, (n, M)).astype(np.int64), rng.integers(5, 90, (n, M, M)).astype(np.int64)
    E, e0 = rng.integers(0, 60, (n, M)).astype(np.int64), rng.integers(0, 60, n).astype(np.int64)
    open_c, close_c, dwell_c = np.zeros(M, np.int64), np.full(M, R.PLAN_TOUR_TICKS_MAX, np.int64), rng.integers(0, 9, M).astype(np.int64)
    open_c[rng.integers(0, M)] = 70
    if hard:
        close_c[rng.permutation(M)[:2]] = rng.integers(90, 200, min(2, M))
        d0[rng.random((n, M)) < 0.15] = NONE
        E[rng.random((n, M)) < 0.1] = NONE
    return dict(d0=d0, D=D, E=E, e0=e0, open_c=open_c, close_c=close_c, dwell_c=dwell_c, t0=int(rng.integers(0, 40)))


def brute_cost(c, r, V):
    """the earliest end of robot r's tour over exactly the stations of the bit set V, by every visit order; None: no feasible one"""
    js = [j for j in range(len(c["open_c"])) if V >> j & 1]
    if not js:
        return None if c["e0"][r] >= NONE else c["t0"] + int(c["e0"][r])
    low = None
    for perm in itertools.permutations(js):
        now, at = c["t0"], -1
        for j in perm:
            leg = c["d0"][r, j] if at < 0 else c["D"][r, at, j]
            begin = max(now + leg, c["open_c"][j])
            if leg >= NONE or begin > c["close_c"][j]:
                break
            now, at = begin + c["dwell_c"][j], j
        else:
            if c["E"][r, at] < NONE and (low is None or now + c["E"][r, at] < low):
                low = int(now + c["E"][r, at])
    return low


def brute_team(c, first, size, T, objective, partial):
    """every assignment of the stations of T to the members (or, with partial, to nobody) -> {covered set: the least (makespan, total)
    or total over the feasible assignments that cover exactly it}"""
    js = [j for j in range(len(c["open_c"])) if T >> j & 1]
    memo = {(k, V): brute_cost(c, first + k, V) for k in range(size) for V in range(1 << len(c["open_c"])) if V & ~T == 0}
    out = {}
    for who in itertools.product(range(size + 1 if partial else size), repeat=len(js)):
        sets = [sum(1 << j for j, w in zip(js, who) if w == k) for k in range(size)]
        each = [memo[k, V] for k, V in enumerate(sets)]
        if any(v is None for v in each):
            continue
        val = (max(each), sum(each)) if objective == "makespan" else (sum(each),)
        cover = sum(sets)
        if cover not in out or val < out[cover]:
            out[cover] = val
    return out, memo


@pytest.mark.parametrize("objective", ["makespan", "sum"])
@pytest.mark.parametrize("partial", [False, True])
@pytest.mark.parametrize("size,M,hard", [(1, 4, True), (2, 5, False), (2, 5, True), (4, 4, True), (4, 5, False), (4, 5, True)])
def test_the_allotment_is_the_brute_force_optimum(size, M, hard, partial, objective):
    teams = 3
    n = teams * size
    c = costs(100 * size + 10 * M + hard, n, M, hard)
    rng = np.random.default_rng(size + M)
    T = np.repeat(rng.integers(1, 1 << M, teams), size)
    T[:size] = (1 << M) - 1
    best = R.spec_plan_best(c["d0"], c["D"], c["E"], c["e0"], c["open_c"], c["close_c"], c["dwell_c"], T, c["t0"])
    share, team = R.spec_plan_share(best, T, size, objective, partial)
    pop = lambda v: bin(int(v)).count("1")   # noqa: E731
    for g in range(teams):
        found, memo = brute_team(c, g * size, size, int(T[g * size]), objective, partial)
        mine = share[g * size:(g + 1) * size]
        for k in range(size):                                            # best is the brute force's cost of every subset
            for V in range(1 << M):
                want = memo.get((k, V))
                assert best[g * size + k, V] == (INF if want is None else want), (g, k, V)
        if not found:
            assert not team["team_feasible"][g] and np.all(mine == 0) and team["team_makespan"][g] == -1 and team["team_total"][g] == -1
            assert team["team_cover"][g] == 0 and team["team_dropped"][g] == T[g * size]
            continue
        assert team["team_feasible"][g]
        cover = int(team["team_cover"][g])
        most = max(pop(u) for u in found)
        assert pop(cover) == most and (partial or cover == T[g * size])           # the number of covered stations first
        low = min(v for u, v in found.items() if pop(u) == most)
        got = (int(team["team_makespan"][g]), int(team["team_total"][g]))
        if objective == "makespan":
            assert got[0] == low[0] and got == found[cover]                      # the value, then (makespan, total) exactly over the cover
            assert partial or got == low
        else:
            assert got[1] == low[0] == found[cover][0]
        assert cover == min(u for u, v in found.items() if pop(u) == most and v[0] == low[0])   # the lowest set of equal values
        assert sum(int(v) for v in mine) == cover and all(int(a) & int(b) == 0 for a, b in itertools.combinations(mine, 2))
        assert team["team_dropped"][g] == T[g * size] & ~cover
        each = [memo[k, int(V)] for k, V in enumerate(mine)]
        assert None not in each and got == (max(each), sum(each))                # a member's cost: its brute-force best for its share
        assert [int(best[g * size + k, int(V)]) for k, V in enumerate(mine)] == each


def test_ties_the_lowest_v_for_the_highest_member():
    pop = np.array([bin(v).count("1") for v in range(8)], np.int64)
    best = np.tile(10 * pop, (4, 1))                                            # every member: 10 a station, in any order
    for objective in ("makespan", "sum"):
        share, team = R.spec_plan_share(best, np.full(4, 7), 4, objective)
        if objective == "makespan":                                             # one station each for three members, the highest with none
            assert share.tolist() == [4, 2, 1, 0] and team["team_makespan"][0] == 10 and team["team_total"][0] == 30
        else:                                                                   # every split costs 30: V = 0 for every member above 0
            assert share.tolist() == [7, 0, 0, 0] and team["team_makespan"][0] == 30 and team["team_total"][0] == 30
    sc = symmetric_scene(n=2)                                                   # both stations 8 cells from both members
    out = R.spec_plan(sc["grid"], None, None, sc["spec"], sc["start"], None, 16, None, share=2)
    assert out["share"].tolist() == [2, 1] and out["cost"].tolist() == [40, 40] and out["team_makespan"][0] == 40
    assert out["tour_order"].tolist() == [[1, -1], [0, -1]] and out["dropped"].tolist() == [0, 0]


def state_with(spec, done):
    st = R.spec_start(done.shape[0], spec)
    cl = R.spec_plan_clauses(spec)
    st.val[:, cl, 0] = np.where(done, np.float32(0.25), st.val[:, cl, 0])
    return st


def plan(sc, **kw):
    return R.spec_plan(sc["grid"], sc["walls"], None, sc["spec"], sc["start"], sc["goal"], 16, sc["pace"], **kw)


@pytest.fixture(scope="module")
def scene():
    return random_scene(1010, 5, S=1, n=8, windows=True, goal=False)


@pytest.mark.parametrize("partial,step0", [(False, 0), (True, 130)])
def test_share_1_is_the_plan_without_share_bit_for_bit(scene, partial, step0):
    rng = np.random.default_rng(3)
    done = rng.integers(0, 2, (8, 5)).astype(bool)
    kw = dict(state=state_with(scene["spec"], done), step0=step0, partial=partial)
    ref = plan(scene, **kw)
    assert not any(k in ref for k in R.SPEC_SHARE_KEYS)                           # share=None is the call it was
    assert partial is False or (np.any(ref["dropped"] != 0) and np.any(ref["status"] == R.PLANNED))
    for objective in ("makespan", "sum"):
        out = plan(scene, share=1, objective=objective, **kw)
        for k in KEYS:
            assert out[k].dtype == ref[k].dtype and np.array_equal(out[k].view(np.uint8), ref[k].view(np.uint8)), (k, objective)
        assert np.array_equal(out["team_done"], done) and np.array_equal(out["share"], np.where(ref["status"] == R.UNREACHABLE, 0, out["team_cover"]))
        assert np.array_equal(out["team_dropped"], ref["dropped"]) and np.array_equal(out["team_makespan"], ref["cost"])


def test_the_members_plans_are_the_replans_of_their_shares_and_nothing_is_vacuous(scene):
    done = np.zeros((8, 5), bool)
    done[1, 3] = True                                                            # a mate's state reads done: T of team 0 has a hole
    st = state_with(scene["spec"], done)
    outs = {o: plan(scene, share=4, objective=o, state=st) for o in ("makespan", "sum")}
    out = outs["makespan"]
    assert out["team_done"].tolist() == [[False, False, False, True, False], [False] * 5]
    assert out["team_cover"].tolist() == [0b10111, 0b11111] and np.all(out["team_feasible"]) and np.all(out["dropped"] == 0)
    for o in outs.values():
        sh = o["share"].reshape(2, 4)
        assert np.array_equal(np.bitwise_or.reduce(sh, axis=1), o["team_cover"]) and np.array_equal(sh.sum(axis=1), o["team_cover"])
        assert np.array_equal(o["cost"].reshape(2, 4).max(axis=1), o["team_makespan"])
        assert np.array_equal(o["cost"].reshape(2, 4).sum(axis=1), o["team_total"])
        alone = plan(scene, state=state_with(scene["spec"], ~((o["share"][:, None] >> np.arange(5)) & 1).astype(bool)))
        for k in R.SPEC_PLAN_KEYS + ("tour_len",):                               # each member: the replan of its share, alone
            assert np.array_equal(o[k].view(np.uint8), alone[k].view(np.uint8)), k
    assert np.all((out["share"].reshape(2, 4) != 0).sum(axis=1) >= 2)            # two or more members with stations
    assert np.any(outs["sum"]["share"] == 0) and np.any(outs["sum"]["status"][outs["sum"]["share"] == 0] == R.PLANNED)   # an empty share
    assert not np.array_equal(out["share"], outs["sum"]["share"])                # the two objectives allot differently
    assert np.all(out["team_makespan"] <= outs["sum"]["team_makespan"]) and np.all(outs["sum"]["team_total"] <= out["team_total"])
    late = plan(scene, share=4, state=st, step0=130)                             # every deadline has closed
    assert not np.any(late["team_feasible"]) and np.all(late["status"] == R.UNREACHABLE) and np.all(late["share"] == 0)
    assert np.all(late["cost"] == -1) and np.all(late["count"] == 0) and np.all(late["tour_order"] == -1) and np.all(late["tour_len"] == 0)
    assert np.array_equal(late["dropped"], np.repeat(late["team_dropped"], 4)) and np.all(late["n_waypoints"] == 0)
    kept = plan(scene, share=4, state=st, step0=130, partial=True)
    assert np.all(kept["team_feasible"]) and np.all(kept["team_dropped"] != 0) and np.all(kept["dropped"] == 0)
    assert np.array_equal(kept["team_cover"] | kept["team_dropped"], [0b10111, 0b11111]) and np.all(kept["status"] == R.PLANNED)


def test_spec_team_result():
    reg = R.Regions([[0.0, 0.0, 0.5, 0.5]], [0])
    spec = R.Spec(reg, [R.Spec.eventually(R.inside(0)), R.Spec.always(R.outside(0)), R.Spec.stay(R.inside(0), 2), R.Spec.recur(R.inside(0), 3),
                        R.Spec.until(R.outside(0), R.inside(0)), R.Spec.eventually(R.inside(0), 50, 60)])
    rho = np.array([[0.1, 0.4, -1.0, 0.3, 0.2, -np.inf], [0.3, 0.2, 0.5, 0.3, 0.7, -np.inf],
                    [0.3, 0.2, 0.5, 0.1, 0.2, -np.inf], [-0.2, 0.9, 0.5, 0.1, 0.9, -np.inf]], np.float32)
    out = R.spec_team_result({"spec_rho": rho}, spec, 4)
    assert out["team_rho"].tolist() == [[np.float32(v) for v in (0.3, 0.2, 0.5, 0.1, 0.2, -np.inf)]]   # max, min, max, min, min, max
    assert out["team_member"].tolist() == [[1, 1, 1, 2, 0, 0]]                   # the lowest member of equal values
    assert out["team_robustness"].tolist() == [-np.inf] and out["team_weakest"].tolist() == [5] and out["team_satisfied"].tolist() == [False]
    pairs = R.spec_team_result({"spec_rho": rho[:, :5]}, R.Spec(reg, spec.clauses[:5]), 2)
    assert pairs["team_rho"].dtype == np.float32 and pairs["team_member"].dtype == np.int32 and pairs["team_weakest"].dtype == np.int32
    assert pairs["team_robustness"].tolist() == [np.float32(0.2), np.float32(0.1)] and pairs["team_weakest"].tolist() == [1, 3]
    assert pairs["team_satisfied"].tolist() == [True, True]
    state = R.spec_start(4, spec)
    state.val[:, :, 0] = rho
    one, ref = R.spec_team_result(R.spec_result(state, spec), spec, 1), R.spec_result(state, spec)
    assert np.array_equal(one["team_rho"].view(np.uint32), ref["spec_rho"].view(np.uint32)) and np.all(one["team_member"] == 0)
    for a, b in (("team_robustness", "robustness"), ("team_weakest", "weakest"), ("team_satisfied", "satisfied")):
        assert one[a].dtype == ref[b].dtype and np.array_equal(one[a], ref[b])
    from mobrob_amd import waypoints
    assert waypoints.spec_team_result({"spec_rho": rho}, spec, 4)["team_member"].tolist() == out["team_member"].tolist()


def test_every_refusal_by_name(scene):
    from mobrob_amd.planning import GridPlanner
    for bad in (3, 0, 32, True, 2.0, "2"):
        with pytest.raises(ValueError, match="share must be a team size"):
            plan(scene, share=bad)
    with pytest.raises(ValueError, match="8 robots do not split into teams of share = 16"):
        plan(scene, share=16)
    for bad in ("max", None, 0):
        with pytest.raises(ValueError, match="objective must be one of"):
            plan(scene, share=2, objective=bad)
    best = np.zeros((8, 32), np.int64)
    with pytest.raises(ValueError, match="share must be a team size"):
        R.spec_plan_share(best, np.zeros(8, np.int64), 3)
    with pytest.raises(ValueError, match="do not split"):
        R.spec_plan_share(best[:6], np.zeros(6, np.int64), 4)
    with pytest.raises(ValueError, match="objective"):
        R.spec_plan_share(best, np.zeros(8, np.int64), 4, "makespan ")
    with pytest.raises(ValueError, match="share one T"):
        R.spec_plan_share(best, np.arange(8), 4)
    spec = scene["spec"]
    with pytest.raises(ValueError, match="size must be one of"):
        R.spec_team_result({"spec_rho": np.zeros((8, spec.n_clauses), np.float32)}, spec, 3)
    with pytest.raises(ValueError, match="do not split into teams"):
        R.spec_team_result({"spec_rho": np.zeros((6, spec.n_clauses), np.float32)}, spec, 4)
    with pytest.raises(ValueError, match="spec_rho must be"):
        R.spec_team_result({"spec_rho": np.zeros((8, spec.n_clauses + 1), np.float32)}, spec, 4)
    # what was refused stays refused, the new keyword or not
    with pytest.raises(ValueError, match="team_size must be 1"):
        plan(dict(scene, spec=R.Spec(spec.regions, spec.clauses, team_size=2)), share=2)
    planner = GridPlanner("point", cells=32, max_waypoints=12, extent=3.0, teams=R.Teams(2, 0.3), layer_steps=4)
    with pytest.raises(ValueError, match="a planner with teams= is not supported"):
        planner.plan_spec(scene["start"], spec, pace=3, share=2)
    host = GridPlanner("point", walls=scene["walls"], cells=32, max_waypoints=16, extent=3.0)
    with pytest.raises(ValueError, match="share must be a team size"):
        host.spec_callback(spec, pace=3, share=3)
    out = host.plan_spec(scene["start"], spec, pace=3, share=4, objective="sum")
    ref = plan(scene, share=4, objective="sum")
    for k in KEYS + R.SPEC_SHARE_KEYS:
        assert np.array_equal(out[k], ref[k]), k


def test_the_specification_callback_replans_a_whole_team(scene):
    from mobrob_amd.planning import GridPlanner
    from mobrob_amd.waypoints import FINISHED, GOING, STALLED, FollowState
    host = GridPlanner("point", walls=scene["walls"], cells=32, max_waypoints=16, extent=3.0)
    run = FollowState(scene["start"], np.zeros((8, 1, 2)), spec=scene["spec"])
    run.spec, run.step0 = R.spec_start(8, scene["spec"]), 0
    status = np.array([GOING, STALLED, FINISHED, GOING, GOING, GOING, FINISHED, GOING])   # team 0 has a stalled member, team 1 none
    ref = host.plan_spec(scene["start"], scene["spec"], pace=3, state=run, partial=True, share=4, objective="sum")
    shared = host.spec_callback(scene["spec"], pace=3, share=4, objective="sum")
    rows = shared(scene["start"], status, np.zeros(8, np.int64), state=run)
    # the whole team of the stalled robot, its finished member and the members without a tour aside; nobody of the other team
    want = [i for i in (0, 1, 3) if ref["status"][i] == R.PLANNED and ref["count"][i] > 0]
    assert sorted(rows) == want and len(want) >= 2 and shared.calls == 1
    for k in KEYS + R.SPEC_SHARE_KEYS:
        assert np.array_equal(shared.last[k], ref[k]), k
    for i in want:
        assert np.array_equal(rows[i][0], ref["waypoints"][i, :ref["count"][i]]) and np.array_equal(rows[i][1], ref["release"][i, :ref["count"][i]])
    alone = host.spec_callback(scene["spec"], pace=3)                            # without share=: the stalled robot only
    assert sorted(alone(scene["start"], status, np.zeros(8, np.int64), state=run)) in ([1], [])
    assert shared(scene["start"], np.full(8, GOING), np.zeros(8, np.int64), state=run) == {} and shared.calls == 2


class _Wander:
    """a policy that needs no checkpoint: a fixed action"""

    def predict(self, obs, deterministic=True):
        return np.array([0.6, 0.3]), None


def test_the_follow_example_shares_and_prints_the_team_verdict(capsys):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mod = importlib.util.spec_from_file_location("follow_cli", os.path.join(root, "examples", "follow.py"))
    cli = importlib.util.module_from_spec(mod)
    mod.loader.exec_module(cli)
    kw = dict(max_steps=40, host=True, seed=3, policy=_Wander(), goal=[0.7, 0.7], plan_cells=64, check_spec=True)
    r = cli.follow("point", "ppo", None, 4, arena=True, plan_spec=True, pace=4, share=2, share_objective="sum", **kw)
    out = capsys.readouterr().out.splitlines()
    assert any(ln.startswith("shared within teams of 2 (sum): 2 of 2 teams allotted, 2 members with stations") for ln in out)
    assert any(ln.startswith("team specification satisfied: ") for ln in out) and any(ln.startswith("worst team robustness: ") for ln in out)
    assert r["team_rho"].shape == (2, 2) and np.array_equal(r["team_rho"][:, 0], r["spec_rho"][:, 0].reshape(2, 2).max(axis=1))
    assert np.sum(r["state"].n_waypoints > 0) == 2 and np.all((r["state"].n_waypoints > 0).reshape(2, 2).sum(axis=1) == 1)   # one member a team
    with pytest.raises(ValueError, match="--share needs --plan-spec"):
        cli.follow("point", "ppo", None, 4, share=2, **kw)
    with pytest.raises(ValueError, match="--share excludes --team-size"):
        cli.follow("point", "ppo", None, 4, plan_spec=True, share=2, team_size=2, **kw)
    with pytest.raises(ValueError, match="--share-objective needs --share"):
        cli.follow("point", "ppo", None, 4, plan_spec=True, share_objective="sum", **kw)
    assert {"share", "share_objective"} <= {a.dest for a in cli.build_parser()._actions}
