"""GPU: the plan from a specification on the device (mobrob_ppo_spec_plan: k_plan_region_occupancy, k_plan_station, k_plan_tour_matrix,
k_plan_tour, k_plan_tour_path, with k_plan_occupancy and k_plan_field as they are) against the NumPy rule (goal_rules.spec_plan), BIT
FOR BIT: every output array, float32 compared as uint32.  Nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest

from mobrob_amd.envs import goal_rules as R
from mobrob_amd.planning import GridPlanner
from tests.plan_spec_scenes import EXTENT, deadline_scene, random_scene, run_rule, symmetric_scene, walled_in_scene
from tests.util import _engine, _env

pytestmark = pytest.mark.gpu
KW = dict(pi=(64, 64), vf=(64, 64))
KEYS = R.SPEC_PLAN_KEYS + ("occupancy", "covered")


@pytest.fixture(scope="module")
def engine():
    e, _ = _engine("point", KW)
    yield e
    e.close()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(dev, ref):
    for k in KEYS:
        assert dev[k].dtype == ref[k].dtype and dev[k].shape == ref[k].shape, (k, dev[k].dtype, dev[k].shape, ref[k].dtype, ref[k].shape)
        bad = np.flatnonzero(bits(dev[k]).ravel() != bits(ref[k]).ravel())
        assert bad.size == 0, f"{k}: {bad.size} of {dev[k].size} entries differ, first at {bad[:5]}"
    assert not np.any(dev["status"] == R.UNCONVERGED) and np.all(dev["sweeps"] > 0)


def device(engine, sc, K=16):
    return engine.plan_spec(sc["grid"], sc["walls"], None, spec=sc["spec"], start=sc["start"], goal=sc["goal"], pace=sc["pace"],
                            max_waypoints=K, want_occupancy=True)


# n robots, M stations, S scenes, P, goal, windows, K: every n with one M at least, the cap of 8 stations (256 subsets), three scenes
# with different counts, both position widths, with and without a goal, a K that truncates
CASES = [(1, 1, 1, 2, False, False, 16), (63, 2, 1, 3, True, True, 16), (65, 7, 3, 2, True, True, 24), (257, 2, 3, 3, False, True, 3),
         (5, 8, 1, 2, True, False, 32), (9, 8, 3, 3, False, True, 4), (33, 1, 3, 2, True, False, 2)]


@pytest.mark.parametrize("n,M,S,P,goal,windows,K", CASES)
def test_g32_every_output_equals_the_rule(engine, n, M, S, P, goal, windows, K):
    sc = random_scene(1000 + 10 * n + M, M, S=S, n=n, windows=windows, pos_dim=P, goal=goal)
    ref = run_rule(sc, K)
    same(device(engine, sc, K), ref)
    assert np.any(ref["status"] != R.UNREACHABLE)                        # a tour exists for some robot: the walk kernel has run
    if K <= 4:
        assert np.any(ref["status"] == R.TRUNCATED)


def test_g64_hazards_and_walls(engine):
    sc = random_scene(77, 4, S=1, n=40, G=64, windows=True, pos_dim=3)
    hz = R.Hazards(np.array([[0.5, 0.5], [-1.0, 1.2]]), size=0.25)
    ref = R.spec_plan(sc["grid"], sc["walls"], hz, sc["spec"], sc["start"], sc["goal"], 24, sc["pace"])
    dev = engine.plan_spec(sc["grid"], sc["walls"], hz, spec=sc["spec"], start=sc["start"], goal=sc["goal"], pace=sc["pace"],
                           max_waypoints=24, want_occupancy=True)
    same(dev, ref)
    assert np.any(ref["release"] != 0)


def test_the_tie_the_walled_in_station_and_the_infeasible_deadline(engine):
    for sc in (symmetric_scene(), walled_in_scene()):
        same(device(engine, sc), run_rule(sc))
    grid, spec, start, goal = deadline_scene()
    for kw in (dict(), dict(deadline=3), dict(deadline=60, opens=400)):
        sc = dict(grid=grid, walls=None, spec=spec(**kw), start=start, goal=goal, pace=2)
        ref = run_rule(sc)
        same(device(engine, sc), ref)
    assert ref["release"].any()


def test_the_planner_on_a_device_env_equals_the_host_path_and_plan_grid_fields_survive(engine):
    sc = random_scene(5, 3, n=16, windows=True, goal=True)
    env = _env("point", 16)
    dev_planner = GridPlanner(env, walls=sc["walls"], cells=32, max_waypoints=12, engine=engine, extent=EXTENT)
    host_planner = GridPlanner("point", walls=sc["walls"], cells=32, max_waypoints=12, extent=EXTENT)
    first = dev_planner.plan(sc["start"], sc["goal"])
    dev = dev_planner.plan_spec(sc["start"], sc["spec"], goal=sc["goal"], pace=3)
    ref = host_planner.plan_spec(sc["start"], sc["spec"], goal=sc["goal"], pace=3)
    for k in R.SPEC_PLAN_KEYS:
        assert np.array_equal(bits(dev[k]), bits(ref[k])), k
    assert (dev["schedule"] is None) == (ref["schedule"] is None)
    again = dev_planner.plan(sc["start"], sc["goal"])                    # a reuse round on the fields resident since `first`
    assert again["fields_reused"]
    for k in ("waypoints", "count", "status", "cost"):
        assert np.array_equal(bits(again[k]), bits(first[k])), k


def test_every_refusal_is_invalid_and_leaves_the_outputs_untouched(engine):
    from mobrob_amd._lib import ERR_INVALID, PlanSpec, SpecC
    n, K, M, G = 4, 4, 2, 32
    grid = R.GridSpec(EXTENT, G)
    i32 = C.POINTER(C.c_int32)
    ip = lambda a: a.ctypes.data_as(i32)   # noqa: E731
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    rows, kinds, counts = np.zeros((1, 3, 4), np.float32), np.zeros((1, 3), np.int32), np.full(1, 3, np.int32)
    rows[0, :, 2:] = 0.4
    start, goal = np.zeros((n, 2), np.float32), np.ones((n, 2), np.float32)
    field_of, fcell, fscene = R.plan_fields(grid, None, None, goal)

    def call(**kw):
        a = dict(n_stations=M, lo=[0, 1], hi=[1, 2], n_avoid=1, alo=[2], ahi=[3], open_c=[0, 0], close_c=[1 << 24, 1 << 24], dwell_c=[0, 0],
                 pace=1, cells=G, n_scenes=1, n_fields=len(fcell), reuse_id=0, goal=goal, kind0=0, r_scenes=1)
        a.update(kw)
        sp = PlanSpec()
        sp.n_robots, sp.pos_dim, sp.cells, sp.max_waypoints, sp.n_scenes, sp.n_fields = n, 2, a["cells"], K, a["n_scenes"], a["n_fields"]
        sp.extent, sp.h, sp.inv_h, sp.inflate, sp.reuse_id = float(grid.extent), float(grid.h), float(grid.inv_h), 0.2, a["reuse_id"]
        rg = SpecC()
        kd = kinds.copy()
        kd[0, 0] = a["kind0"]
        rg.n_scenes, rg.max_regions, rg.n_clauses = a["r_scenes"], 3, 0
        rg.regions, rg.kinds, rg.n_regions, rg.scene = fp(rows), ip(kd), ip(counts), None
        arr = {k: np.array(a[k], np.int32) for k in ("lo", "hi", "alo", "ahi", "open_c", "close_c", "dwell_c")}
        outs = [np.full((n, K, 2), 7, np.float32)] + [np.full(n, 7, np.int32) for _ in range(4)] + [np.full((n, M), 7, np.int32) for _ in range(3)] + \
            [np.full((n, K), 7, np.int32), np.full((1, M), 7, np.int32), np.full((1, M), 7, np.float32), np.full((1, M, M), 7, np.int32)]
        g = a["goal"]
        rc = engine.lib.mobrob_ppo_spec_plan(
            engine._h, C.byref(sp), None, None, C.byref(rg), a["n_stations"], ip(arr["lo"]), ip(arr["hi"]), a["n_avoid"], ip(arr["alo"]),
            ip(arr["ahi"]), ip(arr["open_c"]), ip(arr["close_c"]), ip(arr["dwell_c"]), a["pace"], fp(start), None if g is None else fp(g),
            ip(field_of), ip(fcell), ip(fscene), fp(outs[0]), *(ip(o) for o in outs[1:10]), fp(outs[10]), ip(outs[11]), None, None)
        return rc, outs

    rc, outs = call()
    assert rc == 0 and not any(np.all(o == 7) for o in outs[:9])
    for kw in (dict(n_stations=0), dict(n_stations=9), dict(hi=[1, 4]), dict(lo=[-1, 1]), dict(lo=[2, 1], hi=[1, 2]), dict(ahi=[4]), dict(n_avoid=17),
               dict(open_c=[-1, 0]), dict(dwell_c=[0, (1 << 24) + 1]), dict(close_c=[(1 << 24) + 1, 0]), dict(open_c=[5, 0], close_c=[4, 9]),
               dict(pace=0), dict(cells=48), dict(n_scenes=2), dict(r_scenes=2), dict(reuse_id=5), dict(kind0=2), dict(goal=None),
               dict(n_fields=0), dict(n_fields=n + 1)):
        rc, outs = call(**kw)
        assert rc == ERR_INVALID, kw
        assert all(np.all(o == 7) for o in outs), kw
