"""GPU: smoothing of a team plan on the device (mobrob_ppo_plan_grid_team_smooth: k_plan_occupancy_time, k_plan_team_smooth) against
the NumPy rule (goal_rules.grid_plan_team(smooth=True)), BIT FOR BIT: base layers, every robot's int32 time field, float32 waypoints
compared as uint32, counts, statuses, costs, waits, leave, arrive, release, moves, walks, kept indices and the team clearance.
Nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest

from mobrob_amd.envs import goal_rules as R
from mobrob_amd.envs.goal_rules import GridSpec, Teams, Walls, grid_plan, grid_plan_team
from mobrob_amd.planning import GridPlanner
from mobrob_amd.waypoints import follow_with_replanning
from tests.plan_scenes import EXTENT, INFLATE, SCENE0, robots8_xyz, robots33, serpentine, three_hazards, two_scenes, xyz_checked
from tests.plan_team_scenes import centres, circling32, lattice_case, teams
from tests.plan_team_smooth_cases import rule_scenes, smooth_both
from tests.plan_time_scenes import same_time
from tests.plan_time_smooth_cases import EDGE_ACTIONS, window_edges_waiting
from tests.util import _engine, _env, _snapshot, golden_params, load_golden

pytestmark = pytest.mark.gpu
KW = dict(pi=(64, 64), vf=(64, 64))
PLAN = ("waypoints", "n_waypoints", "count", "status", "cost")
SCENES = rule_scenes()


@pytest.fixture(scope="module")
def engine():
    e, _ = _engine("point", KW)
    yield e
    e.close()


@pytest.mark.parametrize("size", [2, 4, 16])
@pytest.mark.parametrize("r", [0, 1])
@pytest.mark.parametrize("margin", [0, 1])
def test_g32_two_scenes_teams_among_circling_hazards(engine, size, r, margin):
    dev, ref = smooth_both(engine, SCENES[f"circling32_{size}"], 4, r, margin, 8)
    assert {R.PLANNED, R.UNREACHABLE, R.TRUNCATED} <= set(ref["status"].tolist()) and dev["workgroups"] == 32 // size
    both = dev["team_clearance"][dev["team_clearance"] != R.PLAN_NO_PAIR]
    assert both.size and np.all(both > r)


def test_g32_three_column_starts_and_goals_as_teams_of_two(engine):
    spec, walls, hz, start, goal = robots8_xyz()
    _, ref = smooth_both(engine, (spec, walls, hz, start, goal, 2, 10, 8), 4, 1, 0, 8)
    xyz_checked(ref, goal, 4)


def test_g32_without_a_cap_and_with_step0_on_a_hold_table(engine):
    spec, walls, hz, start, goal, size, layer_steps, layers = SCENES["circling32_4"]
    smooth_both(engine, SCENES["circling32_4"], 4, 1, 0, None)
    held = circling32(n_frames=7, frame_steps=4, loop=False)[2]
    smooth_both(engine, (spec, walls, held, start, goal, 4, 5, 8), 4, 1, 1, 8, step0=9)


@pytest.mark.parametrize("max_leg", [None, 8])
def test_head_on_swap(engine, max_leg):
    dev, _ = smooth_both(engine, SCENES["swap"], 8, 1, 0, max_leg)
    assert dev["status"].tolist() == ([R.PLANNED, R.UNREACHABLE] if max_leg is None else [R.PLANNED, R.PLANNED])
    assert dev["team_clearance"].tolist() == [R.PLAN_NO_PAIR if max_leg is None else 2]


@pytest.mark.parametrize("name, r", [("lattice", 2), ("crossing_goal", 1), ("sealed", 1)])
def test_other_g32_scenes(engine, name, r):
    """sealed: a parked earlier member lies on a later member's line"""
    for margin in (0, 1):
        dev, _ = smooth_both(engine, SCENES[name], 16, r, margin, 8)
    if name == "sealed":
        assert dev["status"].tolist() == [R.UNREACHABLE, R.PLANNED] and dev["keeps"][0] == []


def test_cap_one_is_the_unsmoothed_team_plan_on_the_device(engine):
    spec, walls, hz, start, goal, size, layer_steps, layers = SCENES["circling32_4"]
    dev, _ = smooth_both(engine, SCENES["circling32_4"], 64, 1, 1, 1)
    plain = engine.plan_grid_team(spec, walls, hz, teams=teams(4), reserve=1, start=start, goal=goal, layer_steps=layer_steps, layers=layers,
                                  max_waypoints=64, want_fields=True, want_walks=True)
    assert np.array_equal(plain["fields"], dev["fields"]) and plain["walks"] == dev["walks"]
    for k in ("status", "cost", "arrive"):
        assert np.array_equal(plain[k], dev[k]), k


@pytest.mark.parametrize("margin, max_leg", [(0, None), (1, None), (0, 64), (0, 65)])
def test_window_and_ring_edges_as_three_teams_of_two(engine, margin, max_leg):
    """walks of 63, 64, 65, 127, 128 and 129 actions with waits inside; mates are 20 columns apart and never interact; max_leg 64 and
    65: the cap at the edge of a window of 64 candidates"""
    spec, hz, start, goal, layer_steps, layers = window_edges_waiting()
    dev, ref = smooth_both(engine, (spec, None, hz, start, goal, 2, layer_steps, layers), 32, 1, margin, max_leg)
    assert dev["arrive"].tolist() == list(EDGE_ACTIONS) and np.all(dev["status"] == R.PLANNED)
    assert np.all(dev["moves"] < dev["arrive"])


def test_more_teams_than_workgroups(engine):
    """G = 64 and T = 256: a workgroup's scratch is 257 x 64 x 64 x 7 bytes and more, so the 256 MiB cap allows 36 workgroups.  40 teams
    of 2: workgroup 0 takes team 0 and then team 36, on the reservation, walk and kept indices team 0 left behind."""
    spec = GridSpec(EXTENT, 64, INFLATE)
    rng = np.random.default_rng(4)
    start, goal = (rng.uniform(-1.8, 1.8, (80, 2)).astype(np.float32) for _ in range(2))
    goal[78], goal[79] = start[79], start[78]                                    # the last team swaps places
    dev = engine.plan_smooth_team(spec, None, None, teams=teams(2), reserve=1, start=start, goal=goal, layer_steps=10, layers=256, max_waypoints=8,
                                  margin=0, max_leg=8, want_walks=True)
    assert dev["workgroups"] == R.PLAN_TIME_MAX_BYTES // (R.plan_team_smooth_bytes(64, 256) + 4 * ((256 + 64 * 64 + 8) & ~7)) == 36 < 40
    rows = np.array([0, 1, 2, 3, 72, 73, 78, 79])
    ref = grid_plan_team(spec, None, None, start[rows], goal[rows], 8, teams(2), 1, 0, 10, 256, want_fields=False, smooth=True, margin=0, max_leg=8)
    for k in ("waypoints", "n_waypoints", "count", "status", "cost", "waits", "leave", "arrive", "release", "moves"):
        assert np.array_equal(dev[k][rows].view(np.uint32), ref[k].view(np.uint32)), k
    assert [dev["walks"][i] for i in rows] == ref["walks"] and [dev["keeps"][i] for i in rows] == ref["keeps"]
    assert np.array_equal(dev["team_clearance"][[0, 1, 36, 39]], ref["team_clearance"]) and ref["team_clearance"][3] > 1
    assert not np.any(dev["status"] == R.UNCONVERGED)


def test_g128_two_layers_use_the_large_lds_path(engine):
    walls = Walls(SCENE0, radius=0.05)
    start = np.array([[-1.2, -1.2], [1.2, 1.2]], np.float32)
    for margin in (0, 1):
        smooth_both(engine, (GridSpec(EXTENT, 128), walls, None, start, start[::-1].copy(), 2, 20, 2), 12, 2, margin, 8, step0=3)


def test_g64_serpentine_with_both_starts_on_it(engine):
    """margin 1 in a corridor: no cell is clear, every leg is one action, so the fields are the unsmoothed team plan's too; the walks
    and the kept indices are longer than their first buffers, and the engine asks again"""
    spec, walls, start, goal = serpentine()
    start2 = np.concatenate([start, start + np.array([[0.3, 0.0]], np.float32)])
    goal2 = np.tile(goal, (2, 1)) + np.array([[0.0, 0.0], [-0.3, 0.0]], np.float32)
    dev, ref = smooth_both(engine, (spec, walls, None, start2, goal2, 2, 10, 4), 64, 1, 1, 8)
    assert dev["sweeps"].max() > 2 * 64 and dev["arrive"].max() + 1 > 4 + 1 + 2 * 64
    assert dev["keeps"] == [list(range(1, a)) for a in dev["arrive"]]
    plain = engine.plan_grid_team(spec, walls, None, teams=teams(2), reserve=1, start=start2, goal=goal2, layer_steps=10, layers=4, max_waypoints=64,
                                  want_fields=True)
    assert np.array_equal(plain["fields"], dev["fields"])


def test_training_untouched_and_resident_static_fields_survive(engine):
    spec, walls, hz, start, goal = circling32()
    env_a, env_b = _env("point", 16, tl=40), _env("point", 16, tl=40)
    ea, _ = _engine("point", KW, seed=7)
    eb, _ = _engine("point", KW, seed=7)
    scene, st33, gl33 = robots33()
    h3, w33 = three_hazards(scene), two_scenes(scene)
    static = eb.plan_grid(spec, w33, h3, start=st33, goal=gl33, max_waypoints=4)
    for it in range(2):
        env_a.collect(ea)
        env_b.collect(eb)
        before = _snapshot(eb, stats=False)
        got = eb.plan_smooth_team(spec, walls, hz, teams=teams(4), reserve=1, start=start, goal=goal, step0=it, layer_steps=10, layers=8, max_waypoints=4)
        sa, sb = _snapshot(ea, stats=False), _snapshot(eb, stats=False)
        for k in sa:
            assert np.array_equal(sa[k], sb[k]) and np.array_equal(before[k], sb[k]), f"iteration {it}: {k} differs"
        ea.train()
        eb.train()
        assert np.array_equal(ea.get_flat_params(), eb.get_flat_params())
    assert np.any(got["status"] == R.PLANNED)
    moved = st33[::-1].copy()
    again = eb.plan_grid(spec, w33, h3, start=moved, goal=gl33, max_waypoints=4, reuse=static)
    same_time(again, grid_plan(spec, w33, h3, moved, gl33, 4), PLAN)
    assert again["fields_id"] == static["fields_id"]
    ea.close()
    eb.close()


def test_engine_refusals_are_named(engine):
    spec, walls, hz, start, goal = circling32()
    kw = dict(teams=teams(2), reserve=1, start=start, goal=goal, step0=0, layer_steps=10, layers=8, max_waypoints=4)
    for change, word in ((dict(reserve=5), "reserve"), (dict(layers=0), "layers"), (dict(layer_steps=0), "layer_steps"), (dict(step0=-1), "step0"),
                         (dict(max_waypoints=0), "max_waypoints"), (dict(margin=2), "margin"), (dict(max_leg=0), "max_leg"), (dict(max_leg=-1), "max_leg")):
        with pytest.raises(ValueError, match=word):
            engine.plan_smooth_team(spec, walls, hz, **dict(kw, **change))
    with pytest.raises(ValueError, match="one scene"):
        engine.plan_smooth_team(spec, two_scenes(np.arange(32) % 2), None, **kw)
    # the byte cap at its boundary: one workgroup's block of 257 x 128 x 128 x 7 bytes fits, 64 fields of 257 x 128 x 128 x 4 bytes do not
    assert R.plan_team_smooth_bytes(128, 256) <= R.PLAN_TIME_MAX_BYTES < 64 * 257 * 128 * 128 * 4
    with pytest.raises(ValueError, match="exceed the cap"):
        engine.plan_smooth_team(GridSpec(EXTENT, 128), None, None, teams=teams(2), reserve=1, start=np.zeros((64, 2), np.float32),
                                goal=np.zeros((64, 2), np.float32), layer_steps=1, layers=256, want_fields=True)


def test_c_entry_point_refusals_with_hand_made_structs(engine):
    """the checks of mobrob_ppo_plan_grid_team_smooth itself: its own, and through the shared host checks mobrob_ppo_plan_grid_team's"""
    from mobrob_amd import _lib
    spec, walls, hz, start, goal = circling32()
    i32, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)

    def call(n=32, team_size=2, reserve=1, margin=1, max_leg=8, time=(0, 10, 8), keep_cap=0, null_moves=False, **change):
        sp = _lib.PlanSpec()
        sp.n_robots, sp.pos_dim, sp.cells, sp.max_waypoints, sp.n_scenes, sp.n_fields = n, 2, 32, 4, 2, n
        sp.extent, sp.h, sp.inv_h, sp.inflate = float(spec.extent), float(spec.h), float(spec.inv_h), INFLATE
        for k, v in change.items():
            setattr(sp, k, v)
        tm = _lib.PlanTime()
        tm.step0, tm.layer_steps, tm.layers = time
        sc = np.ascontiguousarray(walls.scene[:n], np.int32)
        wl = _lib.WallsC()
        wl.n_scenes, wl.max_walls = walls.n_scenes, walls.max_walls
        wl.boxes, wl.n_walls = walls.table.ctypes.data_as(fp), walls.counts.ctypes.data_as(i32)
        wl.scene, wl.radius, wl.cost, wl.indicator = sc.ctypes.data_as(i32), walls.radius, walls.cost, 1
        wp, rows, out = np.zeros((n, 4, 2), np.float32), [np.zeros((n, 4), np.int32) for _ in range(2)], [np.zeros(n, np.int32) for _ in range(6)]
        keep = np.zeros((n, max(keep_cap, 1)), np.int32)
        return _lib.check(engine.lib.mobrob_ppo_plan_grid_team_smooth(
            engine._h, C.byref(sp), C.byref(wl), None, C.byref(tm), team_size, reserve, margin, max_leg, start.ctypes.data_as(fp),
            goal.ctypes.data_as(fp), wp.ctypes.data_as(fp), *(o.ctypes.data_as(i32) for o in out[:4]), *(o.ctypes.data_as(i32) for o in rows),
            out[4].ctypes.data_as(i32), None if null_moves else out[5].ctypes.data_as(i32), None, None, 0,
            keep.ctypes.data_as(i32) if keep_cap else None, keep_cap, None, None, None))
    assert call() == 0 and call(keep_cap=3) == 0 and call(max_leg=2 ** 31 - 1, margin=0) == 0
    for args, word in ((dict(margin=2), "margin must be 0 or 1"), (dict(margin=-1), "margin must be 0 or 1"), (dict(max_leg=0), "max_leg must be >= 1"),
                       (dict(max_leg=-5), "max_leg must be >= 1"), (dict(null_moves=True), "null argument"),
                       (dict(team_size=3), "team_size must be 1, 2, 4, 8 or 16"), (dict(n=31), "31 robots do not split into teams of 2"),
                       (dict(reserve=5), "reserve must lie in 0 .. 4"), (dict(time=(0, 10, 257)), "layers must lie in 1 .. 256"),
                       (dict(time=(0, 0, 8)), "layer_steps"), (dict(reuse_id=7), "reuse_id"), (dict(cells=48), "cells must be 32, 64 or 128")):
        with pytest.raises(ValueError, match=word):
            call(**args)
    assert call() == 0


def test_closed_loop_three_rounds_with_the_smoothed_team_callback_on_the_device():
    """follow_with_replanning on the reference checkpoint's weights with teams= and the planner's team callback, time_smooth=True, device
    path, against the same plans made by the host rule"""
    e, _ = _engine("point", KW)
    e.set_params(golden_params(load_golden("point")))
    spec, _, _ = lattice_case()
    rng = np.random.default_rng(1)
    lat = np.stack(np.meshgrid(np.arange(32)[4:28:3], np.arange(32)[4:28:3]), axis=-1).reshape(-1, 2)
    cells = lat[rng.choice(len(lat), 64, replace=False)]
    start, goal = centres(spec, cells[:32]), centres(spec, cells[32:])
    tm, r = Teams(4, 0.1), 0
    env = _env("point", 32)
    planner = GridPlanner(env, engine=e, teams=tm, reserve=r, cells=32, inflate=INFLATE, max_waypoints=16, extent=EXTENT, layer_steps=5, layers=48,
                          time_smooth=True, los_margin=0, max_leg=8)
    assert planner.device
    first = planner.plan(start, goal)
    kw = dict(want_fields=False, smooth=True, margin=0, max_leg=8)
    host = grid_plan_team(spec, None, None, start, goal, 16, tm, r, 0, 5, 48, **kw)
    same_time(first, host, ("waypoints", "n_waypoints", "count", "status", "cost", "waits", "leave", "arrive", "release", "moves", "team_clearance"))
    assert first["smoothed"] and first["keeps"] == host["keeps"]
    both = first["team_clearance"][first["team_clearance"] != R.PLAN_NO_PAIR]
    assert both.size and np.all(both > r)
    inner, calls = planner.callback(goal, horizon=20), []

    def recording(positions, status, reached):
        new = inner(positions, status, reached)
        calls.append((new, None if not new else inner.last, positions.copy()))
        return new
    out = follow_with_replanning(e, env, start, first["waypoints"], recording, horizon=20, rounds=3, leg_steps=7, n_waypoints=first["n_waypoints"],
                                 seed=1, teams=tm, schedule=first["schedule"])
    assert len(calls) == 2 and inner.calls == 2 and out["state"].step0 == 60
    assert sum(len(new) for new, _, _ in calls) > 0, "a leg budget of 7 steps stalls robots: the loop must have replanned some"
    for round_, (new, plan, positions) in enumerate(calls, 1):
        if not new:
            continue
        ref = grid_plan_team(spec, None, None, positions.astype(np.float32), goal, 16, tm, r, 20 * round_, 5, 48, **kw)   # step0 = calls * horizon
        same_time(plan, ref, ("waypoints", "n_waypoints", "status", "release", "team_clearance"))
        assert plan["keeps"] == ref["keeps"]
        for i, (w, rel) in new.items():
            assert plan["status"][i] == R.PLANNED and len(w) == plan["n_waypoints"][i] == len(rel)
    e.close()
