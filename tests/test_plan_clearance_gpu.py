"""GPU: clearance-aware grid plans on the device (mobrob_ppo_plan_grid_clear: k_plan_occupancy, k_plan_surcharge, k_plan_field_cost,
k_plan_path_cost; mobrob_ppo_plan_smooth_clear: k_plan_dilate, k_plan_smooth_cost) against the NumPy rule (goal_rules.grid_plan(...,
clearance=)), BIT FOR BIT: surcharge bytes, int32 cost fields, float32 waypoints compared as uint32, counts, statuses, costs, moves,
clearance_min.  Nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest

from mobrob_amd.envs import goal_rules as R
from mobrob_amd.envs.goal_rules import GridSpec, Hazards, Walls, grid_plan
from mobrob_amd.planning import GridPlanner
from tests.plan_scenes import EXTENT, INFLATE, SCENE0, robots33, serpentine, three_hazards, two_scenes
from tests.util import _engine, _env, _snapshot

pytestmark = pytest.mark.gpu
KW = dict(pi=(64, 64), vf=(64, 64))
FULL = ("waypoints", "n_waypoints", "count", "status", "cost", "clearance_min", "occupancy", "surcharge", "fields", "field_of",
        "field_goal_cell", "field_scene")
PATHS = ("waypoints", "n_waypoints", "count", "status", "cost", "clearance_min")


@pytest.fixture(scope="module")
def engine():
    e, _ = _engine("point", KW)
    yield e
    e.close()


def same(dev, ref, keys=FULL):
    for k in keys:
        assert dev[k].dtype == ref[k].dtype and dev[k].shape == ref[k].shape, (k, dev[k].dtype, dev[k].shape, ref[k].dtype, ref[k].shape)
        bad = np.flatnonzero(dev[k].ravel() != ref[k].ravel()) if k != "waypoints" else \
            np.flatnonzero(np.ascontiguousarray(dev[k]).view(np.uint32).ravel() != np.ascontiguousarray(ref[k]).view(np.uint32).ravel())
        assert bad.size == 0, f"{k}: {bad.size} of {dev[k].size} entries differ, first at {bad[:5]}"
    assert not np.any(dev["status"] == R.UNCONVERGED)


def both(engine, spec, walls, hazards, start, goal, K, clearance, scene=None):
    """the plain and the smoothed device plans (both margins) against the rule; -> the plain device dict"""
    ref = grid_plan(spec, walls, hazards, start, goal, K, clearance=clearance)
    dev = engine.plan_grid_clear(spec, walls, hazards, clearance=clearance, start=start, goal=goal, max_waypoints=K, want_occupancy=True,
                                 want_fields=True, want_surcharge=True)
    same(dev, ref)
    for margin in (0, 1):
        sref = grid_plan(spec, walls, hazards, start, goal, K, occupancy=ref["occupancy"], fields=ref["fields"], smooth=True, margin=margin,
                         clearance=clearance)
        sdev = engine.plan_smooth_clear(spec, reuse=dev, start=start, goal=goal, scene=scene, max_waypoints=K, margin=margin)
        same(sdev, sref, PATHS + ("moves",))
    return dev, ref


@pytest.mark.parametrize("clearance", [(1, 1), (2, 8), (8, 16)])
@pytest.mark.parametrize("scene_kind", ["walls", "walls_hazards", "hazards", "empty"])
def test_g32_two_scenes_33_robots(engine, scene_kind, clearance):
    scene, start, goal = robots33()
    walls = two_scenes(scene) if scene_kind.startswith("walls") else None
    hazards = three_hazards(scene) if "hazards" in scene_kind else None
    if scene_kind == "empty":
        hazards = Hazards(np.zeros((0, 2)))
    spec = GridSpec(EXTENT, 32, INFLATE if walls is not None else None)
    dev, ref = both(engine, spec, walls, hazards, start, goal, 4, clearance, scene=None if scene_kind == "empty" else scene)
    assert np.all((dev["sweeps"] >= 1) & (dev["sweeps"] <= 32 * 32))
    assert np.all((ref["clearance_min"] == -1) == (ref["status"] == R.UNREACHABLE))
    if scene_kind == "empty":
        assert not dev["surcharge"].any() and np.all(dev["clearance_min"] == clearance[0] + 1)
    else:
        assert dev["surcharge"].max() == clearance[0] * clearance[1]
    if scene_kind == "walls" and clearance == (8, 16):
        free = ~ref["occupancy"]
        assert np.all(ref["surcharge"][free] > 0) and ref["surcharge"].max() == 128      # every free cell lies within reach of a wall
        assert set(ref["status"].tolist()) == {R.PLANNED, R.UNREACHABLE, R.TRUNCATED}


def test_g128_uses_the_96_kb_lds_path(engine):
    rng = np.random.default_rng(5)
    walls = Walls(SCENE0, radius=0.05)
    goals = np.array([(1.2, 1.2), (-1.2, -1.2), (1.2, -1.3), (-0.3, 1.3)], np.float32)     # the third lies in the sealed pocket
    start = rng.uniform(-1.5, 1.5, (9, 2)).astype(np.float32)
    goal = goals[np.arange(9) % 4]
    spec = GridSpec(EXTENT, 128)
    dev, ref = both(engine, spec, walls, None, start, goal, 12, (4, 6))
    assert len(ref["field_goal_cell"]) == 4 and np.any(ref["status"] == R.PLANNED) and np.any(ref["status"] == R.UNREACHABLE)


def test_g64_serpentine_long_convergence(engine):
    spec, walls, start, goal = serpentine()
    dev, ref = both(engine, spec, walls, None, start, goal, 64, (2, 8))
    plain = engine.plan_grid(spec, walls, None, start=start, goal=goal, max_waypoints=64)
    print("serpentine sweeps with surcharges:", dev["sweeps"], "plain:", plain["sweeps"], "cost:", dev["cost"], "plain:", plain["cost"])
    assert ref["status"][0] == R.PLANNED and dev["sweeps"][0] >= 0 and dev["cost"][0] >= plain["cost"][0]


def test_k2_grow_replanning_rounds_and_the_two_families(engine):
    scene, start, goal = robots33()
    walls = two_scenes(scene)
    env = _env("point", 33)
    clearance = (2, 8)
    planner = GridPlanner(env, walls=walls, cells=32, inflate=INFLATE, max_waypoints=2, engine=engine, extent=EXTENT, clearance=clearance)
    spec = planner.spec
    ref2 = grid_plan(spec, walls, None, start, goal, 2, clearance=clearance)
    got = planner.plan(start, goal, want_occupancy=True, want_fields=True)
    same(got, ref2, tuple(k for k in FULL if k != "surcharge"))
    assert np.any(got["status"] == R.TRUNCATED) and not got["fields_reused"] and got["clearance"] == clearance
    grown = planner.plan(start, goal, grow=True)
    full = grid_plan(spec, walls, None, start, goal, int(ref2["count"].max()), clearance=clearance)
    same(grown, full, PATHS)
    assert grown["waypoints"].shape[1] == ref2["count"].max() > 2 and not np.any(grown["status"] == R.TRUNCATED)
    # a replanning round on the resident cost fields: new starts, the same goals; plain and smoothed at both margins
    moved = start[::-1].copy()
    again = planner.plan(moved, goal)
    assert again["fields_reused"]
    same(again, grid_plan(spec, walls, None, moved, goal, 2, clearance=clearance), PATHS)
    kept = dict(planner._kept)
    for margin in (0, 1):
        sm = GridPlanner(env, walls=walls, cells=32, inflate=INFLATE, max_waypoints=6, engine=engine, extent=EXTENT, clearance=clearance,
                         smooth=True, los_margin=margin)
        first = sm.plan(start, goal)
        second = sm.plan(moved, goal)
        assert not first["fields_reused"] and second["fields_reused"]
        same(first, grid_plan(spec, walls, None, start, goal, 6, smooth=True, margin=margin, clearance=clearance), PATHS + ("moves",))
        same(second, grid_plan(spec, walls, None, moved, goal, 6, smooth=True, margin=margin, clearance=clearance), PATHS + ("moves",))
    # the callback of a replanning loop plans on the resident clearance fields
    from mobrob_amd.waypoints import STALLED
    cb = sm.callback(goal)
    rows = cb(moved, np.full(33, STALLED), np.zeros(33, bool))
    assert cb.last["fields_reused"] and cb.last["clearance"] == clearance and len(rows) > 0
    # the two families stay resident side by side; an id of the other family is a state error either way round
    plain = engine.plan_grid(spec, walls, None, start=start, goal=goal, max_waypoints=2)
    clear = engine.plan_grid_clear(spec, walls, None, clearance=clearance, start=start, goal=goal, max_waypoints=2)
    same(engine.plan_grid(spec, walls, None, start=moved, goal=goal, max_waypoints=2, reuse=plain),
         grid_plan(spec, walls, None, moved, goal, 2), ("waypoints", "n_waypoints", "count", "status", "cost"))
    same(engine.plan_grid_clear(spec, walls, None, clearance=clearance, start=moved, goal=goal, max_waypoints=2, reuse=clear),
         grid_plan(spec, walls, None, moved, goal, 2, clearance=clearance), PATHS)
    from mobrob_amd._lib import EngineError
    for call in (lambda: engine.plan_grid_clear(spec, walls, None, clearance=clearance, start=start, goal=goal, max_waypoints=2, reuse=plain),
                 lambda: engine.plan_smooth_clear(spec, reuse=plain, start=start, goal=goal, scene=scene, max_waypoints=2),
                 lambda: engine.plan_grid(spec, walls, None, start=start, goal=goal, max_waypoints=2, reuse=clear),
                 lambda: engine.plan_smooth(spec, reuse=clear, start=start, goal=goal, scene=scene, max_waypoints=2),
                 lambda: engine.plan_grid_clear(spec, walls, None, clearance=clearance, start=start, goal=goal, max_waypoints=2, reuse=kept)):
        with pytest.raises(EngineError, match=r"\[-3\]"):                         # MOBROB_ERR_STATE
            call()
    with pytest.raises(ValueError, match="reach, weight"):
        engine.plan_grid_clear(spec, walls, None, clearance=(3, 8), start=start, goal=goal, max_waypoints=2, reuse=clear)


def test_refusals_are_named(engine):
    from mobrob_amd import _lib
    scene, start, goal = robots33()
    walls = two_scenes(scene)
    spec = GridSpec(EXTENT, 32, INFLATE)
    for bad in ((0, 1), (9, 1), (1, 0), (1, 17), (True, 1)):
        with pytest.raises(ValueError, match="clearance"):
            engine.plan_grid_clear(spec, walls, None, clearance=bad, start=start, goal=goal)
    with pytest.raises(ValueError, match="max_waypoints"):
        engine.plan_grid_clear(spec, walls, None, clearance=(2, 8), start=start, goal=goal, max_waypoints=0)
    with pytest.raises(ValueError, match="finite"):
        engine.plan_grid_clear(spec, walls, None, clearance=(2, 8), start=np.where(np.arange(33)[:, None] == 2, np.inf, start), goal=goal)
    ok = engine.plan_grid_clear(spec, walls, None, clearance=(2, 8), start=start, goal=goal, max_waypoints=4)
    i32, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)

    def call(reach=2, weight=8, **change):
        sp = _lib.PlanSpec()
        sp.n_robots, sp.pos_dim, sp.cells, sp.max_waypoints, sp.n_scenes, sp.n_fields = 33, 2, 32, 4, 2, len(ok["field_goal_cell"])
        sp.extent, sp.h, sp.inv_h, sp.inflate = float(spec.extent), float(spec.h), float(spec.inv_h), INFLATE
        fof, fcell, fscene = ok["field_of"].copy(), ok["field_goal_cell"].copy(), ok["field_scene"].copy()
        for k, v in change.items():
            if k == "field_of":
                fof[0] = v
            elif k == "field_goal_cell":
                fcell[0] = v
            else:
                setattr(sp, k, v)
        wl = _lib.WallsC()
        wl.n_scenes, wl.max_walls = walls.n_scenes, walls.max_walls
        wl.boxes, wl.n_walls = walls.table.ctypes.data_as(fp), walls.counts.ctypes.data_as(i32)
        wl.scene, wl.radius, wl.cost, wl.indicator = walls.scene.ctypes.data_as(i32), walls.radius, walls.cost, 1
        wp, out = np.zeros((33, 4, 2), np.float32), [np.zeros(33, np.int32) for _ in range(5)]
        return _lib.check(engine.lib.mobrob_ppo_plan_grid_clear(
            engine._h, C.byref(sp), C.byref(wl), None, reach, weight, start.ctypes.data_as(fp), goal.ctypes.data_as(fp),
            fof.ctypes.data_as(i32), fcell.ctypes.data_as(i32), fscene.ctypes.data_as(i32), wp.ctypes.data_as(fp),
            *(o.ctypes.data_as(i32) for o in out), None, None, None, None, None))
    assert call() == 0
    for kw, word in ((dict(reach=0), "reach must lie in 1 .. 8"), (dict(reach=9), "reach"), (dict(weight=0), "weight must lie in 1 .. 16"),
                     (dict(weight=17), "weight"), (dict(cells=48), "cells must be 32, 64 or 128"), (dict(max_waypoints=0), "max_waypoints"),
                     (dict(pos_dim=1), "pos_dim"), (dict(n_scenes=3), "n_scenes"), (dict(inv_h=7.0), "h \\* inv_h"), (dict(inflate=-1.0), "inflate"),
                     (dict(field_of=99), "field_of\\[0\\]"), (dict(field_goal_cell=1024), "field_goal_cell\\[0\\]"),
                     (dict(field_goal_cell=0), "goal of robot"), (dict(n_fields=0), "n_fields"), (dict(n_robots=0), "n_robots")):
        with pytest.raises(ValueError, match=word):
            call(**kw)
    with pytest.raises(ValueError, match="margin"):
        engine.plan_smooth_clear(spec, reuse=ok, start=start, goal=goal, scene=scene, max_waypoints=4, margin=2)
    same(engine.plan_grid_clear(spec, walls, None, clearance=(2, 8), start=start, goal=goal, max_waypoints=4), ok, PATHS)


def test_training_untouched_by_clearance_calls():
    scene, start, goal = robots33()
    walls = two_scenes(scene)
    spec = GridSpec(EXTENT, 32, INFLATE)
    env_a, env_b = _env("point", 16, tl=40), _env("point", 16, tl=40)
    ea, _ = _engine("point", KW, seed=7)
    eb, _ = _engine("point", KW, seed=7)
    kept = None
    for it in range(2):
        env_a.collect(ea)
        env_b.collect(eb)
        before = _snapshot(eb, stats=False)
        kept = eb.plan_grid_clear(spec, walls, three_hazards(scene), clearance=(2, 8), start=start, goal=goal, max_waypoints=4, want_fields=True)
        eb.plan_grid_clear(spec, walls, three_hazards(scene), clearance=(2, 8), start=start[::-1].copy(), goal=goal, max_waypoints=4, reuse=kept)
        eb.plan_smooth_clear(spec, reuse=kept, start=start, goal=goal, scene=scene, max_waypoints=4, margin=1)
        sa, sb = _snapshot(ea, stats=False), _snapshot(eb, stats=False)
        for k in sa:
            assert np.array_equal(sa[k], sb[k]) and np.array_equal(before[k], sb[k]), f"iteration {it}: {k} differs"
        ea.train()
        eb.train()
        assert np.array_equal(ea.get_flat_params(), eb.get_flat_params())
    assert np.any(kept["status"] == R.PLANNED)
    ea.close()
    eb.close()
