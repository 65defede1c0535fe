"""GPU: line-of-sight smoothing of a time plan on the device (mobrob_ppo_plan_grid_time_smooth: k_plan_next_blocked, k_plan_smooth_time,
and k_plan_dilate over the layers at margin 1) against the NumPy rule (goal_rules.grid_plan_time(smooth=True)), BIT FOR BIT: layer
maps, int32 time fields, the int16 next-blocked table, float32 waypoints compared as uint32, counts, statuses, costs, leave,
release, arrive and moves.  Nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest

from mobrob_amd.envs import goal_rules as R
from mobrob_amd.envs.goal_rules import GridSpec, MovingHazards, grid_plan_time
from mobrob_amd.planning import GridPlanner
from mobrob_amd.waypoints import follow_with_replanning
from tests.plan_scenes import EXTENT, INFLATE, robots8_xyz, serpentine, xyz_checked
from tests.plan_smooth_cases import same_plan
from tests.plan_time_scenes import FAR, circling33, gap_case, goal_sitter, same_time
from tests.plan_time_smooth_cases import EDGE_ACTIONS, EDGE_MOVES, SMOOTH_KEYS, cap_boundary, static_twin, window_edges_waiting
from tests.util import _engine, _env, _snapshot, golden_params, load_golden

pytestmark = pytest.mark.gpu
KW = dict(pi=(64, 64), vf=(64, 64))
ALL = SMOOTH_KEYS + ("occupancy", "fields", "next_blocked")


@pytest.fixture(scope="module")
def engine():
    e, _ = _engine("point", KW)
    yield e
    e.close()


def both(engine, spec, walls, hz, start, goal, K, step0, layer_steps, layers, margin):
    ref = grid_plan_time(spec, walls, hz, start, goal, K, step0, layer_steps, layers, smooth=True, margin=margin, want_next_blocked=True)
    dev = engine.plan_smooth_time(spec, walls, hz, start=start, goal=goal, step0=step0, layer_steps=layer_steps, layers=layers, max_waypoints=K,
                                  margin=margin, want_occupancy=True, want_fields=True, want_next_blocked=True)
    same_time(dev, ref, ALL)
    assert not np.any(dev["status"] == R.UNCONVERGED) and np.all(dev["sweeps"] >= 1)
    return dev, ref


@pytest.mark.parametrize("margin", [0, 1])
@pytest.mark.parametrize("layer_steps,layers", [(3, 64), (10, 32)])
def test_g32_two_scenes_33_robots_loop_and_hold(engine, layer_steps, layers, margin):
    spec, walls, hz, scene, start, goal = circling33()
    dev, ref = both(engine, spec, walls, hz, start, goal, 64, 0, layer_steps, layers, margin)
    print("circling33", (layer_steps, layers), "margin", margin, "count", int(dev["count"].sum()), "arrive > moves:", int(np.sum(dev["arrive"] > dev["moves"])))
    gone = ref["status"] == R.UNREACHABLE
    assert gone.sum() == 10 and not dev["waypoints"][gone].any() and not dev["leave"][gone].any() and np.all(dev["count"][gone] == 0)
    assert layer_steps == 3 or np.any(ref["arrive"] > ref["moves"]), "at 10 steps a layer some walks wait"
    held = circling33(n_frames=7, frame_steps=4, loop=False)[2]
    both(engine, spec, walls, held, start, goal, 64, 9, layer_steps, layers, margin)      # step0 > 0; the tail holds the last frame


def test_g32_three_column_starts_and_goals(engine):
    spec, walls, hz, start, goal = robots8_xyz()
    _, ref = both(engine, spec, walls, hz, start, goal, 4, 0, 10, 8, 0)
    xyz_checked(ref, goal, 4)


@pytest.mark.parametrize("margin", [0, 1])
def test_gap_case_and_goal_sitter(engine, margin):
    spec, walls, hz, start, goal = gap_case()
    dev, ref = both(engine, spec, walls, hz, start, goal, 64, 0, 10, 16, margin)
    assert ref["arrive"][0] == 9 and ref["moves"][0] == 7                              # two waits in the walk
    spec, hz, start, goal = goal_sitter()
    dev, ref = both(engine, spec, None, hz, start, goal, 64, 0, 10, 16, margin)
    assert dev["count"][0] == 2 and dev["release"][0, 1] > 0                             # the goal is blocked in the early layers


def test_g128_serpentine_with_a_wait_wraps_the_ring_many_times(engine):
    spec, walls, start, goal = serpentine(cells=128)
    lane = float(start[0, 1])
    hz = MovingHazards(np.array([[[0.0, lane]], [FAR]]), size=0.05, frame_steps=300)      # sits in the first lane for 300 steps (60 layers), then parks
    for margin in (0, 1):
        dev, ref = both(engine, spec, walls, hz, start, goal, 64, 0, 5, 64, margin)
        print("serpentine 128 margin", margin, "arrive", dev["arrive"], "moves", dev["moves"], "count", dev["count"])
        assert ref["arrive"][0] > 4 * 128 and ref["arrive"][0] > ref["moves"][0], "the ring wraps, and the walk waits for the hazard to leave its lane"


def test_window_edges_63_64_65_127_128_129_actions_with_waits_inside(engine):
    spec, hz, start, goal, layer_steps, layers = window_edges_waiting()
    for margin in (0, 1):
        dev, ref = both(engine, spec, None, hz, start, goal, 32, 0, layer_steps, layers, margin)
        assert ref["arrive"].tolist() == list(EDGE_ACTIONS) and ref["moves"].tolist() == list(EDGE_MOVES)   # (the cases' docstring says why)
        assert np.all(ref["status"] == R.PLANNED) and np.all(ref["count"] >= 2)


def test_t4_walks_far_past_the_tail(engine):
    spec, walls, hz, scene, start, goal = circling33()
    for margin in (0, 1):
        dev, ref = both(engine, spec, walls, hz, start, goal, 64, 0, 3, 4, margin)
        assert np.sum(ref["arrive"] > 20) >= 1


def test_truncation_grow_and_the_unsmoothed_bits_on_the_planner(engine):
    spec, walls, hz, scene, start, goal = circling33()
    env = _env("point", 33)
    kw = dict(walls=walls, hazards=hz, cells=32, inflate=INFLATE, engine=engine, extent=EXTENT, layer_steps=10, layers=8)
    planner = GridPlanner(env, max_waypoints=2, time_smooth=True, los_margin=0, **kw)
    ref2 = grid_plan_time(spec, walls, hz, start, goal, 2, 0, 10, 8, smooth=True, margin=0)
    got = planner.plan(start, goal, want_occupancy=True, want_fields=True)
    same_time(got, ref2, SMOOTH_KEYS + ("occupancy", "fields"))
    assert np.any(got["status"] == R.TRUNCATED) and got["smoothed"] and not got["fields_reused"]
    grown = planner.plan(start, goal, grow=True)
    full = grid_plan_time(spec, walls, hz, start, goal, int(ref2["count"].max()), 0, 10, 8, smooth=True, margin=0)
    same_time(grown, full, SMOOTH_KEYS)
    assert grown["waypoints"].shape[1] == ref2["count"].max() > 2 and np.array_equal(grown["schedule"].release, full["release"])
    # time_smooth=False: the bits of plan_grid_time, from the same planner and from one without the keyword
    today = engine.plan_grid_time(spec, walls, hz, start=start, goal=goal, step0=0, layer_steps=10, layers=8, max_waypoints=2)
    raw = ("waypoints", "n_waypoints", "count", "status", "cost", "waits", "leave", "arrive", "release")
    same_time(today, grid_plan_time(spec, walls, hz, start, goal, 2, 0, 10, 8), raw)
    for p in (planner.plan(start, goal, time_smooth=False), GridPlanner(env, max_waypoints=2, **kw).plan(start, goal)):
        same_time(p, today, raw)
        assert not p["smoothed"] and p["moves"] is None


@pytest.mark.parametrize("margin", [0, 1])
def test_one_frame_equals_plan_smooth_of_the_same_engine(engine, margin):
    spec, walls, one, h3, start, goal = static_twin()
    full = engine.plan_grid(spec, walls, h3, start=start, goal=goal, max_waypoints=64)
    static = engine.plan_smooth(spec, reuse=full, start=start, goal=goal, scene=R.plan_scene(walls, h3)[1], max_waypoints=64, margin=margin)
    timed = engine.plan_smooth_time(spec, walls, one, start=start, goal=goal, step0=5, layer_steps=3, layers=5, max_waypoints=64, margin=margin)
    same_plan(timed, static)
    moved = start[::-1].copy()                                                   # the static fields are still resident
    again = engine.plan_smooth(spec, reuse=full, start=moved, goal=goal, scene=R.plan_scene(walls, h3)[1], max_waypoints=64, margin=margin)
    assert again["fields_id"] == full["fields_id"] and np.any(again["status"] == R.PLANNED)


def test_refusals_are_named_before_any_launch(engine):
    from mobrob_amd import _lib
    spec, walls, hz, scene, start, goal = circling33()
    kw = dict(start=start, goal=goal, step0=0, layer_steps=10, layers=8, max_waypoints=4)
    ok = engine.plan_smooth_time(spec, walls, hz, margin=0, **kw)
    for change, word in ((dict(margin=2), "margin must be 0 or 1"), (dict(margin=True), "margin must be 0 or 1"), (dict(layers=0), "layers"),
                         (dict(layers=257), "layers"), (dict(layer_steps=0), "layer_steps"), (dict(step0=-1), "step0"),
                         (dict(step0=2 ** 31 - 90), "fit an int32"), (dict(max_waypoints=0), "max_waypoints")):
        with pytest.raises(ValueError, match=word):
            engine.plan_smooth_time(spec, walls, hz, **dict(dict(kw, margin=0), **change))
    with pytest.raises(TypeError, match="MovingHazards"):
        engine.plan_smooth_time(spec, walls, None, **kw)
    # the cap at its boundary: 15 fields over 2 scenes at G = 128, T = 256 fit alone (240.9 MiB) and not with the table (257.0 MiB)
    bspec, bhz, bstart, bgoal, bls, bT = cap_boundary()
    with pytest.raises(ValueError, match="next-blocked table"):
        engine.plan_smooth_time(bspec, None, bhz, start=bstart, goal=bgoal, layer_steps=bls, layers=bT, max_waypoints=2)
    R.plan_time_smooth_check(15, 1, bT, 128, 1)                                  # one scene's table fits: the table term is what refuses
    # the C entry point's own checks, reached with hand-made structs
    i32, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)

    def call(margin=0, time=(0, 10, 8), null_moves=False, fields=None, **change):
        sp = _lib.PlanSpec()
        sp.n_robots, sp.pos_dim, sp.cells, sp.max_waypoints, sp.n_scenes, sp.n_fields = 33, 2, 32, 4, 2, len(ok["field_goal_cell"])
        sp.extent, sp.h, sp.inv_h, sp.inflate = float(spec.extent), float(spec.h), float(spec.inv_h), INFLATE
        for k, v in change.items():
            setattr(sp, k, v)
        tm = _lib.PlanTime()
        tm.step0, tm.layer_steps, tm.layers = time
        h, keep = engine._hazards_struct(hz, 33)
        wl = _lib.WallsC()
        wl.n_scenes, wl.max_walls = walls.n_scenes, walls.max_walls
        wl.boxes, wl.n_walls = walls.table.ctypes.data_as(fp), walls.counts.ctypes.data_as(i32)
        wl.scene, wl.radius, wl.cost, wl.indicator = walls.scene.ctypes.data_as(i32), walls.radius, walls.cost, 1
        wp, rows, out = np.zeros((33, 4, 2), np.float32), [np.zeros((33, 4), np.int32) for _ in range(2)], [np.zeros(33, np.int32) for _ in range(6)]
        return _lib.check(engine.lib.mobrob_ppo_plan_grid_time_smooth(
            engine._h, C.byref(sp), C.byref(wl), C.byref(h), C.byref(tm), margin, start.ctypes.data_as(fp), goal.ctypes.data_as(fp),
            ok["field_of"].ctypes.data_as(i32), ok["field_goal_cell"].ctypes.data_as(i32), ok["field_scene"].ctypes.data_as(i32),
            wp.ctypes.data_as(fp), *(o.ctypes.data_as(i32) for o in out[:4]), None, rows[1].ctypes.data_as(i32), out[4].ctypes.data_as(i32),
            None if null_moves else out[5].ctypes.data_as(i32), None, None, None, None))
    assert call() == 0 and call(margin=1) == 0                                   # (waits_out may be NULL)

    def call_boundary(smooth):
        """the engine's own cap check at cap_boundary's shape: the same arguments to both entry points, no walls, K = 2"""
        fof, fcell, fscene = R.plan_fields(bspec, None, bhz.scene, bgoal)
        sp = _lib.PlanSpec()
        sp.n_robots, sp.pos_dim, sp.cells, sp.max_waypoints, sp.n_scenes, sp.n_fields = 15, 2, 128, 2, 2, len(fcell)
        sp.extent, sp.h, sp.inv_h, sp.inflate = float(bspec.extent), float(bspec.h), float(bspec.inv_h), float(bspec.inflate_for(None))
        tm = _lib.PlanTime()
        tm.step0, tm.layer_steps, tm.layers = 0, bls, bT
        h, keep = engine._hazards_struct(bhz, 15)
        wp, rows, out = np.zeros((15, 2, 2), np.float32), [np.zeros((15, 2), np.int32) for _ in range(2)], [np.zeros(15, np.int32) for _ in range(6)]
        head = (engine._h, C.byref(sp), None, C.byref(h), C.byref(tm))
        robots = (bstart.ctypes.data_as(fp), bgoal.ctypes.data_as(fp), fof.ctypes.data_as(i32), fcell.ctypes.data_as(i32), fscene.ctypes.data_as(i32),
                  wp.ctypes.data_as(fp), *(o.ctypes.data_as(i32) for o in out[:4]), *(o.ctypes.data_as(i32) for o in rows), out[4].ctypes.data_as(i32))
        if smooth:
            return _lib.check(engine.lib.mobrob_ppo_plan_grid_time_smooth(*head, 0, *robots, out[5].ctypes.data_as(i32), None, None, None, None)), out
        return _lib.check(engine.lib.mobrob_ppo_plan_grid_time(*head, *robots, None, None, None)), out
    assert len(R.plan_fields(bspec, None, bhz.scene, bgoal)[1]) == 15
    rc, out = call_boundary(False)                                               # the fields alone fit: the unsmoothed call plans
    assert rc == 0 and np.all(out[2] == R.PLANNED)
    with pytest.raises(ValueError, match="next-blocked table of 2 x 257 x 128 x 128 x 2"):
        call_boundary(True)
    for args, word in ((dict(margin=2), "margin must be 0 or 1"), (dict(margin=-1), "margin must be 0 or 1"), (dict(null_moves=True), "null argument"),
                       (dict(time=(0, 10, 0)), "layers must lie in 1 .. 256"), (dict(time=(0, 0, 8)), "layer_steps"), (dict(time=(-1, 10, 8)), "step0"),
                       (dict(reuse_id=7), "reuse_id"), (dict(cells=48), "cells must be 32, 64 or 128"), (dict(max_waypoints=0), "max_waypoints"),
                       (dict(n_scenes=3), "n_scenes"), (dict(inflate=-1.0), "inflate")):
        with pytest.raises(ValueError, match=word):
            call(**args)
    same_time(engine.plan_smooth_time(spec, walls, hz, margin=0, **kw), ok, SMOOTH_KEYS)     # a refused call changes nothing


def test_training_untouched_by_smoothed_time_plans():
    spec, walls, hz, scene, start, goal = circling33()
    env_a, env_b = _env("point", 16, tl=40), _env("point", 16, tl=40)
    ea, _ = _engine("point", KW, seed=7)
    eb, _ = _engine("point", KW, seed=7)
    for it in range(2):
        env_a.collect(ea)
        env_b.collect(eb)
        before = _snapshot(eb, stats=False)
        for margin in (0, 1):
            got = eb.plan_smooth_time(spec, walls, hz, start=start, goal=goal, step0=it, layer_steps=10, layers=8, max_waypoints=4, margin=margin,
                                      want_next_blocked=True)
        sa, sb = _snapshot(ea, stats=False), _snapshot(eb, stats=False)
        for k in sa:
            assert np.array_equal(sa[k], sb[k]) and np.array_equal(before[k], sb[k]), f"iteration {it}: {k} differs"
        ea.train()
        eb.train()
        assert np.array_equal(ea.get_flat_params(), eb.get_flat_params())
    assert np.any(got["status"] == R.PLANNED)
    ea.close()
    eb.close()


def test_replanning_loop_equals_the_loop_driven_by_the_host_rule():
    e, _ = _engine("point", KW)
    e.set_params(golden_params(load_golden("point")))
    rng = np.random.default_rng(3)
    spec, walls, hz, _, _ = gap_case(stay=30)
    start = rng.uniform(-1.4, 1.4, (32, 2)).astype(np.float32)
    start[:, 0] = -np.abs(start[:, 0]) - 0.15                                    # left of the thin wall, goals right of it
    goal = np.tile(np.array([[1.2, 1.2], [1.3, -0.2]], np.float32), (16, 1))
    kw = dict(walls=walls, hazards=hz, cells=32, inflate=INFLATE, max_waypoints=16, extent=EXTENT, layer_steps=5, layers=16, time_smooth=True,
              los_margin=0)
    runs = []
    for device in (True, False):
        env = _env("point", 32)
        planner = GridPlanner(env, engine=e, **kw) if device else GridPlanner("point", **kw)
        assert planner.device == device
        first = planner.plan(start, goal)
        inner, calls = planner.callback(goal, horizon=20), []

        def recording(positions, status, reached, inner=inner, calls=calls):
            new = inner(positions, status, reached)
            calls.append(new)
            return new
        out = follow_with_replanning(e, env, start, first["waypoints"], recording, horizon=20, rounds=3, leg_steps=7, n_waypoints=first["n_waypoints"],
                                     seed=1, hazards=hz, walls=walls, schedule=first["schedule"])
        assert len(calls) == 2 and inner.calls == 2 and out["state"].step0 == 60
        runs.append((first, calls, out))
    (fa, ca, oa), (fb, cb, ob) = runs
    same_time(fa, fb, SMOOTH_KEYS)
    assert fa["smoothed"] and np.any(fa["release"] > 0)
    assert sum(len(c) for c in ca) > 0, "a leg budget of 7 steps stalls robots: the loop must have replanned some"
    for new_a, new_b in zip(ca, cb):
        assert sorted(new_a) == sorted(new_b)
        for i in new_a:
            assert new_a[i][0].view(np.uint32).tobytes() == new_b[i][0].view(np.uint32).tobytes() and np.array_equal(new_a[i][1], new_b[i][1])
    for k in ("arrival", "reached", "status", "steps", "hold_steps", "cost_sum", "round_status"):
        assert np.array_equal(oa[k], ob[k], equal_nan=oa[k].dtype.kind == "f"), k
    assert np.array_equal(oa["state"].release, ob["state"].release) and np.array_equal(oa["state"].waypoints, ob["state"].waypoints)
    e.close()
