"""GPU: the plan from a specification from the middle of a run on the device (mobrob_ppo_spec_replan: k_plan_tour_resume,
k_plan_tour_path_legs after the kernels mobrob_ppo_spec_plan runs) against the NumPy rule (goal_rules.spec_plan with state=, step0=,
partial=), BIT FOR BIT: every output array, the three new ones included, float32 compared as uint32.  Nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest

from mobrob_amd.envs import goal_rules as R
from mobrob_amd.planning import GridPlanner
from tests.plan_spec_scenes import EXTENT, random_scene
from tests.util import _engine, _env

pytestmark = pytest.mark.gpu
KW = dict(pi=(64, 64), vf=(64, 64))
KEYS = R.SPEC_PLAN_KEYS + R.SPEC_REPLAN_KEYS + ("occupancy", "covered")
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


def todo_pattern(which, n, M, seed):
    """-> done bool [n][M]: all done, none done, a single station left, random per robot (robot 0 with nothing left, robot 1 with
    everything, robot 2 -- where a station has a deadline -- with only that one left)"""
    rng = np.random.default_rng(seed)
    if which == "all":
        return np.ones((n, M), bool)
    if which == "none":
        return np.zeros((n, M), bool)
    if which == "single":
        done = np.ones((n, M), bool)
        done[np.arange(n), rng.integers(0, M, n)] = False
        return done
    done = rng.integers(0, 2, (n, M)).astype(bool)
    done[0] = True
    if n > 1:
        done[1] = False
    timed = [j for j in range(M) if (j + seed) % 4 == 0]
    if n > 2 and timed:
        done[2] = True
        done[2, timed[0]] = False
    return done


def both(engine, sc, K, hz=None, **kw):
    ref = R.spec_plan(sc["grid"], sc["walls"], hz, sc["spec"], sc["start"], sc["goal"], K, sc["pace"], **kw)
    dev = engine.plan_spec(sc["grid"], sc["walls"], hz, spec=sc["spec"], start=sc["start"], goal=sc["goal"], pace=sc["pace"],
                           max_waypoints=K, want_occupancy=True, **kw)
    same(dev, ref)
    return ref


# n robots, M stations, S scenes, P, goal, K: 63 and 65 straddle a wave, 257 a workgroup of 16-lane groups; the cap of 8 stations;
# K = 3 and 4 truncate
CASES = [(1, 1, 1, 2, False, 16), (63, 2, 1, 3, True, 16), (65, 7, 3, 2, True, 24), (257, 2, 3, 3, False, 3), (9, 8, 3, 3, True, 4),
         (257, 8, 1, 2, True, 4)]
VARIANTS = [("none", 0, False), ("all", LATE, False), ("single", 0, True), ("random", LATE, True), ("random", LATE, False)]


@pytest.mark.parametrize("which,step0,partial", VARIANTS)
@pytest.mark.parametrize("n,M,S,P,goal,K", CASES)
def test_g32_every_output_equals_the_rule(engine, n, M, S, P, goal, K, which, step0, partial):
    seed = 1000 + 10 * n + M
    sc = random_scene(seed, M, S=S, n=n, windows=True, pos_dim=P, goal=goal)
    done = todo_pattern(which, n, M, seed)
    ref = both(engine, sc, K, state=state_with(sc["spec"], done), step0=step0, partial=partial)
    assert np.array_equal(ref["done"], done)
    if which == "none":
        assert np.any(ref["tour_len"] == M)                                 # a full tour for some robot: both kernels have run
        if K <= 4 and n > 200:                                              # the two places the prefix-sum emission can go wrong
            cut = ref["status"] == R.TRUNCATED
            at_station = np.any(ref["station_waypoint"] == K - 1, axis=1)
            assert np.any(cut & at_station) and np.any(cut & ~at_station)
    if which == "all":
        assert np.all(ref["tour_len"] == 0) and (goal or np.all(ref["count"] == 0))
    if which == "random" and partial and M >= 4 and n > 8:                  # not vacuous: dropped, kept all, ended with nothing
        todo = (~done).astype(int) @ (1 << np.arange(M))
        assert np.any(ref["dropped"] != 0) and np.any((todo != 0) & (ref["dropped"] == 0) & (ref["status"] != R.UNREACHABLE))
        assert np.any((todo != 0) & (ref["tour_len"] == 0) & (ref["status"] != R.UNREACHABLE)) or not goal


def test_g64_hazards_and_walls(engine):
    sc = random_scene(77, 4, S=1, n=40, G=64, windows=True, pos_dim=3)
    hz = R.Hazards(np.array([[0.5, 0.5], [-1.0, 1.2]]), size=0.25)
    done = todo_pattern("random", 40, 4, 77)
    ref = both(engine, sc, 24, hz=hz, state=state_with(sc["spec"], done), step0=40, partial=True)
    assert np.any(ref["tour_len"] > 1)


def direct(engine, name, sc, K, todo=None, t0=0, partial=0, poison=None, **bad):
    """one call of mobrob_ppo_spec_plan or mobrob_ppo_spec_replan itself -> (rc, outputs by name)"""
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
    sp.n_robots, sp.pos_dim, sp.cells, sp.max_waypoints, sp.n_scenes, sp.n_fields = n, P, G, K, S, len(fcell)
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
             matrix=fill((S, M, M), np.int32), tour_len=fill(n, np.int32), dropped=fill(n, np.int32))
    ins = [engine._h, C.byref(sp), None, None, C.byref(rg), M, ip(lo), ip(hi), len(avoid), ip(alo), ip(ahi), ip(open_c), ip(close_c), ip(dwell_c),
           pace, fp(start), fp(goal), ip(field_of), ip(fcell), ip(fscene)]
    outs = [fp(o["waypoints"])] + [ip(o[k]) for k in ("n_waypoints", "count", "status", "cost", "tour_order", "tour_eta", "station_waypoint",
                                                      "release", "station_cell")] + [fp(o["station_margin"]), ip(o["matrix"]), None, None]
    if name == "mobrob_ppo_spec_plan":
        return engine.lib.mobrob_ppo_spec_plan(*ins, *outs), o
    todo = np.full(n, (1 << M) - 1, np.int32) if todo is None else np.ascontiguousarray(todo, np.int32)
    more = [ip(o["tour_len"]), ip(o["dropped"])]
    if "null" in bad:
        todo, more = (None, more) if bad["null"] == 0 else (todo, [None if q + 1 == bad["null"] else m for q, m in enumerate(more)])
    return engine.lib.mobrob_ppo_spec_replan(*ins, ip(todo), t0, partial, *outs, *more), o


def test_the_new_entry_point_at_its_defaults_is_the_old_one(engine):
    sc = random_scene(1657, 7, S=3, n=65, windows=True, goal=True, walls=False)
    rc0, old = direct(engine, "mobrob_ppo_spec_plan", sc, 24)
    rc1, new = direct(engine, "mobrob_ppo_spec_replan", sc, 24)
    assert rc0 == 0 and rc1 == 0
    for k in old:
        if k not in ("tour_len", "dropped"):
            assert np.array_equal(bits(old[k]), bits(new[k])), k
    planned = old["status"] != R.UNREACHABLE
    assert np.any(planned) and np.array_equal(new["tour_len"], np.where(planned, 7, 0)) and np.array_equal(new["dropped"], np.where(planned, 0, 127))


def test_every_new_refusal_is_invalid_and_leaves_the_outputs_untouched(engine):
    from mobrob_amd._lib import ERR_INVALID
    sc = random_scene(5, 3, n=4, windows=True, goal=True, walls=False)
    rc, outs = direct(engine, "mobrob_ppo_spec_replan", sc, 4, poison=7)
    assert rc == 0 and not any(np.all(o == 7) for k, o in outs.items() if k not in ("station_cell", "station_margin", "matrix"))
    top = R.PLAN_TOUR_TICKS_MAX
    for kw in (dict(t0=-1), dict(t0=top + 1), dict(partial=2), dict(partial=-1), dict(todo=[7, 7, 8, 7]), dict(todo=[0, -1, 0, 0]),
               dict(todo=[1 << 30, 0, 0, 0]), dict(null=0), dict(null=1), dict(null=2)):
        rc, outs = direct(engine, "mobrob_ppo_spec_replan", sc, 4, poison=7, **kw)
        assert rc == ERR_INVALID, kw
        assert all(np.all(o == 7) for o in outs.values()), kw
    assert direct(engine, "mobrob_ppo_spec_replan", sc, 4, t0=top, partial=1, todo=[7, 0, 1, 6])[0] == 0


def test_the_planner_on_a_device_env_equals_the_host_path_and_plan_grid_fields_survive(engine):
    from mobrob_amd.waypoints import FollowState
    sc = random_scene(5, 3, n=16, windows=True, goal=True)
    env = _env("point", 16)
    dev_planner = GridPlanner(env, walls=sc["walls"], cells=32, max_waypoints=12, engine=engine, extent=EXTENT)
    host_planner = GridPlanner("point", walls=sc["walls"], cells=32, max_waypoints=12, extent=EXTENT)
    assert dev_planner.device and not host_planner.device
    first = dev_planner.plan(sc["start"], sc["goal"])
    run = FollowState(sc["start"], np.zeros((16, 1, 2)), spec=sc["spec"])
    run.step0 = 45
    run.spec = state_with(sc["spec"], todo_pattern("random", 16, 3, 5))
    for partial in (False, True):
        dev = dev_planner.plan_spec(sc["start"], sc["spec"], goal=sc["goal"], pace=3, state=run, partial=partial)
        ref = host_planner.plan_spec(sc["start"], sc["spec"], goal=sc["goal"], pace=3, state=run, partial=partial)
        for k in R.SPEC_PLAN_KEYS + R.SPEC_REPLAN_KEYS:
            assert np.array_equal(bits(dev[k]), bits(ref[k])), k
        assert dev["t0"] == ref["t0"] == 75 and (dev["schedule"] is None) == (ref["schedule"] is None)
    again = dev_planner.plan(sc["start"], sc["goal"])                    # a reuse round on the fields resident since `first`
    assert again["fields_reused"]
    for k in ("waypoints", "count", "status", "cost"):
        assert np.array_equal(bits(again[k]), bits(first[k])), k


def test_one_replanning_round_with_the_specification_callback(engine):
    from mobrob_amd.waypoints import FollowState, follow_with_replanning
    sc = random_scene(5, 3, n=16, windows=True, goal=False)
    env = _env("point", 16)
    planner = GridPlanner(env, walls=sc["walls"], cells=32, max_waypoints=12, engine=engine, extent=EXTENT)
    host = GridPlanner("point", walls=sc["walls"], cells=32, max_waypoints=12, extent=EXTENT)
    first = planner.plan_spec(sc["start"], sc["spec"], pace=3, partial=True)
    inner, seen = planner.spec_callback(sc["spec"], pace=3, when="all"), []

    def recording(positions, status, reached, state=None):
        rows = inner(positions, status, reached, state=state)
        seen.append((positions.copy(), status.copy(), state.copy(), rows))
        return rows
    recording.wants_state = True
    follow_with_replanning(engine, env, sc["start"], first["waypoints"], recording, horizon=20, rounds=2, n_waypoints=first["n_waypoints"],
                           schedule=R.Schedule(first["release"], home=sc["start"]), spec=sc["spec"], path_stride=1)
    assert len(seen) == 1 and inner.calls == 1
    positions, status, state, rows = seen[0]
    assert isinstance(state, FollowState) and isinstance(state.spec, R.SpecState) and state.step0 == 20
    ref = host.plan_spec(positions, sc["spec"], pace=3, state=state, partial=True)
    same(inner.last, ref, R.SPEC_PLAN_KEYS + R.SPEC_REPLAN_KEYS)
    from mobrob_amd.waypoints import FINISHED
    want = [i for i in range(16) if status[i] != FINISHED and ref["status"][i] == R.PLANNED and ref["count"][i] > 0]
    assert sorted(rows) == want and len(want) > 0
    for i in want:
        assert np.array_equal(bits(rows[i][0]), bits(ref["waypoints"][i, :ref["count"][i]])) and np.array_equal(rows[i][1], ref["release"][i, :ref["count"][i]])
