"""GPU: a team shares the stations of a specification on the device (mobrob_ppo_spec_plan_share: k_plan_tour_best, k_plan_team_share,
k_plan_tour_resume over the shares, k_plan_team_void, k_plan_tour_path_legs) against the NumPy rule (goal_rules.spec_plan with share=
and objective=), BIT FOR BIT: every output array, float32 compared as uint32.  Nothing here has a tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest

from mobrob_amd.envs import goal_rules as R
from mobrob_amd.planning import GridPlanner
from tests.plan_spec_scenes import EXTENT, random_scene
from tests.util import _engine, _env

pytestmark = pytest.mark.gpu
KW = dict(pi=(64, 64), vf=(64, 64))
TEAM_KEYS = R.SPEC_SHARE_KEYS + ("team_feasible",)
KEYS = R.SPEC_PLAN_KEYS + R.SPEC_REPLAN_KEYS + TEAM_KEYS + ("occupancy", "covered")
LATE = 130   # a step by which every deadline of random_scene (below step 120) has closed


@pytest.fixture(scope="module")
def engine():
    e, _ = _engine("point", KW)
    yield e
    e.close()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(dev, ref, keys=KEYS):
    for k in keys:
        assert dev[k].dtype == ref[k].dtype and dev[k].shape == ref[k].shape, (k, dev[k].dtype, dev[k].shape, ref[k].dtype, ref[k].shape)
        bad = np.flatnonzero(bits(dev[k]).ravel() != bits(ref[k]).ravel())
        assert bad.size == 0, f"{k}: {bad.size} of {dev[k].size} entries differ, first at {bad[:5]}"
    assert not np.any(dev["status"] == R.UNCONVERGED) and np.all(dev["sweeps"] > 0) and dev["t0"] == ref["t0"]


def state_with(spec, done):
    st = R.spec_start(done.shape[0], spec)
    cl = R.spec_plan_clauses(spec)
    st.val[:, cl, 0] = np.where(done, np.float32(0.25), st.val[:, cl, 0])
    return st


def holes(n, M, size, seed):
    """-> done bool [n][M].  Teams of one: one station in five done.  Larger teams in turn: nothing done (T is every station), some
    stations done for member 0 only, some for the last two members -- so that T is full for a third of the teams and holed for the
    rest, whatever the team size (a station is done for the team once it is for ANY member)"""
    rng = np.random.default_rng(seed)
    if size == 1:
        return rng.random((n, M)) < 0.2
    done = np.zeros((n, M), bool)
    for g in range(n // size):
        for k in ((), (0,), (size - 2, size - 1))[g % 3]:
            done[g * size + k] = rng.random(M) < 0.25
            done[g * size + k, rng.integers(0, M)] = True
    return done


def both(engine, sc, K, hz=None, **kw):
    ref = R.spec_plan(sc["grid"], sc["walls"], hz, sc["spec"], sc["start"], sc["goal"], K, sc["pace"], **kw)
    dev = engine.plan_spec(sc["grid"], sc["walls"], hz, spec=sc["spec"], start=sc["start"], goal=sc["goal"], pace=sc["pace"],
                           max_waypoints=K, want_occupancy=True, **kw)
    same(dev, ref)
    return ref


# size, n robots, M stations, S scenes, P, goal, K, extra variants: every team size; M = 8 at the sizes 2, 4, 8 and 16 (T = 255: the
# 3^8 submask loop, the full 256-entry rows, sixteen real costs in a sum) and M = 1, M = 5; one team of 16; 64 + size and 256 + 16 robots
# straddle a wave and a workgroup of the per-robot kernels; K = 3 truncates.  Every case runs ("makespan", 0, False) and ("sum", LATE,
# True); the other variants are dealt over the cases, so that the NumPy rule is not run more often than the coverage needs.
BASE = [("makespan", 0, False), ("sum", LATE, True)]
CASES = [(1, 65, 5, 3, 2, True, 16, [("sum", 0, False)]), (2, 66, 8, 1, 3, False, 16, [("makespan", LATE, False), ("sum", 0, False)]),
         (4, 68, 8, 1, 2, True, 16, [("makespan", LATE, True)]), (4, 68, 1, 1, 2, True, 16, []), (8, 72, 8, 3, 3, True, 3, [("makespan", LATE, True)]),
         (16, 16, 8, 1, 2, False, 16, [("sum", 0, False), ("makespan", LATE, True)]), (16, 80, 5, 3, 2, True, 24, [("makespan", LATE, False)]),
         (16, 272, 8, 1, 3, True, 16, [])]
RUNS = [c[:7] + v for c in CASES for v in BASE + c[7]]


@functools.lru_cache(maxsize=None)
def scene_for(size, n, M, S, P, goal):
    """-> (scene, state, done), made once per case.  Mates start near each other and share the goal of their first member; teams of 4
    and more plan on an open map: a member whose start or goal lies in an obstacle leaves its whole team without an allotment"""
    seed = 2000 + 10 * n + M + {16: 2, 80: 1}.get(n, 0)   # seeds at which the teams of 16 reach their stations before the deadlines
    free = size >= 4
    sc = random_scene(seed, M, S=S, n=n, windows=True, pos_dim=P, goal=goal, walls=not free, n_avoid=0 if free else 2)
    if size > 1:
        lead = np.arange(n) // size * size
        sc["start"] = (sc["start"][lead] + np.random.default_rng(seed).uniform(-0.3, 0.3, sc["start"].shape)).astype(np.float32).clip(-2.9, 2.9)
        if goal:
            sc["goal"] = np.ascontiguousarray(sc["goal"][lead])
    done = holes(n, M, size, seed)
    return sc, state_with(sc["spec"], done), done


@pytest.mark.parametrize("size,n,M,S,P,goal,K,objective,step0,partial", RUNS)
def test_g32_every_output_equals_the_rule(engine, size, n, M, S, P, goal, K, objective, step0, partial):
    sc, state, done = scene_for(size, n, M, S, P, goal)
    ref = both(engine, sc, K, state=state.copy(), step0=step0, partial=partial, share=size, objective=objective)
    pop = np.array([bin(int(v)).count("1") for v in ref["team_cover"]])
    sh = ref["share"].reshape(n // size, size)
    assert np.array_equal(ref["team_done"], done.reshape(n // size, size, M).any(axis=1))
    if step0 == 0:                                                               # not vacuous, on the rule's own output
        assert size == 1 or 2 * ref["team_feasible"].sum() > n // size           # most teams have an allotment
        assert n // size < 3 or size == 1 or (np.any(ref["team_done"].any(axis=1) & ref["team_feasible"]) and np.any(~ref["team_done"].any(axis=1) & ref["team_feasible"]))
        if M == 8:
            assert np.any(pop == 8)                                              # a team that covers all eight: U = 255 on the device
            assert np.any((sh != 0).sum(axis=1) >= min(size, 4 if objective == "makespan" else 2))   # and one with several members on the way
            assert size == 1 or np.any((ref["share"] == 0) & (ref["status"] == R.PLANNED))
        if size == 2:
            assert np.any(ref["tour_len"] > 2)
    elif partial:
        assert (M == 1 or np.any(ref["team_dropped"] != 0)) and np.any(ref["team_feasible"])
    else:
        assert np.any(~ref["team_feasible"])


def test_g64_hazards_and_walls(engine):
    sc = random_scene(77, 4, S=1, n=40, G=64, windows=True, pos_dim=3)
    hz = R.Hazards(np.array([[0.5, 0.5], [-1.0, 1.2]]), size=0.25)
    ref = both(engine, sc, 24, hz=hz, state=state_with(sc["spec"], holes(40, 4, 4, 77)), step0=40, partial=True, share=4)
    assert np.any((ref["share"].reshape(10, 4) != 0).sum(axis=1) >= 2) and np.any(ref["team_feasible"])   # a team that shares


def direct(engine, name, sc, K, todo=None, t0=0, partial=0, size=1, objective=0, poison=None, null=None, n_robots=None):
    """one call of mobrob_ppo_spec_replan or mobrob_ppo_spec_plan_share itself -> (rc, outputs by name)"""
    from mobrob_amd._lib import PlanSpec, SpecC
    grid, spec, start, goal = sc["grid"], sc["spec"], np.ascontiguousarray(sc["start"], np.float32), np.ascontiguousarray(sc["goal"], np.float32)
    avoid, stations, (open_c, close_c, dwell_c), S, scene, _, _, _, pace = R.spec_plan_check(grid, None, None, spec, start, goal, K, sc["pace"])
    n, P = start.shape
    M, G, reg = len(stations), grid.cells, spec.regions
    i32 = C.POINTER(C.c_int32)
    ip = lambda a: None if a is None else a.ctypes.data_as(i32)   # noqa: E731
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    field_of, fcell, fscene = R.plan_fields(grid, None, scene, goal)
    sp = PlanSpec()
    sp.n_robots, sp.pos_dim, sp.cells, sp.max_waypoints, sp.n_scenes, sp.n_fields = n if n_robots is None else n_robots, P, G, K, S, len(fcell)
    sp.extent, sp.h, sp.inv_h, sp.inflate, sp.reuse_id = float(grid.extent), float(grid.h), float(grid.inv_h), float(grid.inflate_for(None)), 0
    rg = SpecC()
    rg.n_scenes, rg.max_regions, rg.n_clauses = reg.n_scenes, reg.max_regions, 0
    rg.regions, rg.kinds, rg.n_regions, rg.scene = fp(reg.table), ip(reg.kinds), ip(reg.counts), ip(reg.scene)
    lo, hi = (np.array([s[k] for s in stations], np.int32) for k in (0, 1))
    alo, ahi = (np.array([a[k] for a in avoid], np.int32) for k in (0, 1))
    fill = (lambda shape, dt: np.zeros(shape, dt)) if poison is None else (lambda shape, dt: np.full(shape, poison, dt))
    o = dict(waypoints=fill((n, K, P), np.float32), n_waypoints=fill(n, np.int32), count=fill(n, np.int32), status=fill(n, np.int32),
             cost=fill(n, np.int32), tour_order=fill((n, M), np.int32), tour_eta=fill((n, M), np.int32), station_waypoint=fill((n, M), np.int32),
             release=fill((n, K), np.int32), station_cell=fill((S, M), np.int32), station_margin=fill((S, M), np.float32),
             matrix=fill((S, M, M), np.int32), tour_len=fill(n, np.int32), dropped=fill(n, np.int32), share=fill(n, np.int32),
             team_cover=fill(n, np.int32), team_dropped=fill(n, np.int32), team_makespan=fill(n, np.int32), team_total=fill(n, np.int64))
    ins = [engine._h, C.byref(sp), None, None, C.byref(rg), M, ip(lo), ip(hi), len(avoid), ip(alo), ip(ahi), ip(open_c), ip(close_c), ip(dwell_c),
           pace, fp(start), fp(goal), ip(field_of), ip(fcell), ip(fscene)]
    outs = [fp(o["waypoints"])] + [ip(o[k]) for k in ("n_waypoints", "count", "status", "cost", "tour_order", "tour_eta", "station_waypoint",
                                                      "release", "station_cell")] + [fp(o["station_margin"]), ip(o["matrix"]), None, None]
    todo = np.full(n, (1 << M) - 1, np.int32) if todo is None else np.ascontiguousarray(todo, np.int32)
    more = [ip(o["tour_len"]), ip(o["dropped"])]
    if name == "mobrob_ppo_spec_replan":
        return engine.lib.mobrob_ppo_spec_replan(*ins, ip(todo), t0, partial, *outs, *more), o
    team = [ip(o[k]) for k in ("share", "team_cover", "team_dropped", "team_makespan")] + [o["team_total"].ctypes.data_as(C.POINTER(C.c_int64))]
    team = [None if q == null else m for q, m in enumerate(team)]
    return engine.lib.mobrob_ppo_spec_plan_share(*ins, ip(todo), t0, partial, size, objective, *outs, *more, *team), o


@pytest.mark.parametrize("partial,t0", [(0, 0), (1, 220)])
def test_team_size_1_is_the_replan_call_for_both_objectives(engine, partial, t0):
    sc = random_scene(1657, 7, S=3, n=65, windows=True, goal=True, walls=False)
    todo = np.random.default_rng(5).integers(0, 128, 65).astype(np.int32)
    rc0, old = direct(engine, "mobrob_ppo_spec_replan", sc, 24, todo=todo, t0=t0, partial=partial)
    assert rc0 == 0 and np.any(old["status"] == R.PLANNED) and (not partial or np.any(old["dropped"] != 0))
    for objective in (0, 1):
        rc1, new = direct(engine, "mobrob_ppo_spec_plan_share", sc, 24, todo=todo, t0=t0, partial=partial, objective=objective)
        assert rc1 == 0
        for k in old:
            if not k.startswith("team_") and k != "share":
                assert np.array_equal(bits(old[k]), bits(new[k])), (k, objective)
        assert np.array_equal(new["team_dropped"], old["dropped"]) and np.array_equal(new["team_makespan"], old["cost"])
        assert np.array_equal(new["share"], np.where(old["status"] == R.UNREACHABLE, 0, todo & ~old["dropped"]))


def test_every_new_refusal_is_invalid_and_leaves_the_outputs_untouched(engine):
    from mobrob_amd._lib import ERR_INVALID
    sc = random_scene(5, 3, n=4, windows=True, goal=True, walls=False)
    rc, outs = direct(engine, "mobrob_ppo_spec_plan_share", sc, 4, size=2, poison=7)
    # every output is written by a good call (team_cover aside: a team that covers all three stations reads 7 itself)
    assert rc == 0 and not any(np.all(o == 7) for k, o in outs.items() if k not in ("station_cell", "station_margin", "matrix", "team_cover"))
    assert np.all(outs["team_cover"][:2] == (outs["share"][0::2] | outs["share"][1::2])[:2])
    for kw in (dict(size=0), dict(size=3), dict(size=32), dict(size=-1), dict(size=8), dict(size=2, n_robots=3), dict(size=2, objective=2),
               dict(size=2, objective=-1), dict(size=2, null=0), dict(size=2, null=1), dict(size=2, null=2), dict(size=2, null=3), dict(size=2, null=4),
               dict(size=2, partial=2), dict(size=2, todo=[8, 0, 0, 0])):
        rc, outs = direct(engine, "mobrob_ppo_spec_plan_share", sc, 4, poison=7, **kw)
        assert rc == ERR_INVALID, kw
        assert all(np.all(o == 7) for o in outs.values()), kw
    assert direct(engine, "mobrob_ppo_spec_plan_share", sc, 4, size=4, objective=1, partial=1, todo=[7, 0, 1, 6])[0] == 0


def test_the_planner_on_a_device_env_equals_the_host_path_and_plan_grid_fields_survive(engine):
    sc = random_scene(5, 3, n=16, windows=True, goal=True)
    env = _env("point", 16)
    dev_planner = GridPlanner(env, walls=sc["walls"], cells=32, max_waypoints=12, engine=engine, extent=EXTENT)
    host_planner = GridPlanner("point", walls=sc["walls"], cells=32, max_waypoints=12, extent=EXTENT)
    assert dev_planner.device and not host_planner.device
    first = dev_planner.plan(sc["start"], sc["goal"])
    state = state_with(sc["spec"], holes(16, 3, 4, 5))
    for objective, partial in (("makespan", False), ("sum", True)):
        kw = dict(goal=sc["goal"], pace=3, state=state, step0=45, partial=partial, share=4, objective=objective)
        dev, ref = dev_planner.plan_spec(sc["start"], sc["spec"], **kw), host_planner.plan_spec(sc["start"], sc["spec"], **kw)
        for k in R.SPEC_PLAN_KEYS + R.SPEC_REPLAN_KEYS + TEAM_KEYS:
            assert np.array_equal(bits(dev[k]), bits(ref[k])), k
        assert dev["t0"] == ref["t0"] == 75 and (dev["schedule"] is None) == (ref["schedule"] is None)
    again = dev_planner.plan(sc["start"], sc["goal"])                    # a reuse round on the fields resident since `first`
    assert again["fields_reused"]
    for k in ("waypoints", "count", "status", "cost"):
        assert np.array_equal(bits(again[k]), bits(first[k])), k
