"""GPU: prioritised planning inside a team on the device (mobrob_ppo_plan_grid_team: k_plan_occupancy_time, k_plan_team) against the
NumPy rule (goal_rules.grid_plan_team), BIT FOR BIT: base layers, every robot's int32 time field, float32 waypoints compared as
uint32, counts, statuses, costs, waits, leave, arrive, release, walks and the team clearance.  Nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest

from mobrob_amd.envs import goal_rules as R
from mobrob_amd.envs.goal_rules import GridSpec, Teams, Walls, grid_plan, grid_plan_team
from mobrob_amd.planning import GridPlanner
from mobrob_amd.waypoints import follow_with_replanning
from tests.plan_scenes import EXTENT, INFLATE, SCENE0, robots8_xyz, robots33, serpentine, three_hazards, two_scenes, xyz_checked
from tests.plan_team_scenes import centres, circling32, lattice_case, same_team, swap_case, teams
from tests.plan_time_scenes import same_time
from tests.util import _engine, _env, _snapshot, golden_params, load_golden

pytestmark = pytest.mark.gpu
KW = dict(pi=(64, 64), vf=(64, 64))
PLAN = ("waypoints", "n_waypoints", "count", "status", "cost")


@pytest.fixture(scope="module")
def engine():
    e, _ = _engine("point", KW)
    yield e
    e.close()


def both(engine, spec, walls, hz, start, goal, K, size, r, step0, layer_steps, layers):
    ref = grid_plan_team(spec, walls, hz, start, goal, K, teams(size), r, step0, layer_steps, layers)
    dev = engine.plan_grid_team(spec, walls, hz, teams=teams(size), reserve=r, start=start, goal=goal, step0=step0, layer_steps=layer_steps,
                                layers=layers, max_waypoints=K, want_occupancy=True, want_fields=True, want_walks=True)
    same_team(dev, ref)
    assert dev["walks"] == ref["walks"]
    assert not np.any(dev["status"] == R.UNCONVERGED) and np.all(dev["sweeps"] >= 1)
    return dev, ref


@pytest.mark.parametrize("size", [2, 4, 16])
@pytest.mark.parametrize("r", [0, 1])
def test_g32_two_scenes_teams_among_circling_hazards(engine, size, r):
    spec, walls, hz, start, goal = circling32()
    dev, ref = both(engine, spec, walls, hz, start, goal, 4, size, r, 0, 10, 8)
    assert {R.PLANNED, R.UNREACHABLE, R.TRUNCATED} <= set(ref["status"].tolist()) and dev["workgroups"] == 32 // size


def test_g32_three_column_starts_and_goals_as_teams_of_two(engine):
    spec, walls, hz, start, goal = robots8_xyz()
    _, ref = both(engine, spec, walls, hz, start, goal, 4, 2, 1, 0, 10, 8)
    xyz_checked(ref, goal, 4)


def test_g32_step0_on_a_hold_table(engine):
    spec, walls, _, start, goal = circling32()
    held = circling32(n_frames=7, frame_steps=4, loop=False)[2]
    both(engine, spec, walls, held, start, goal, 4, 4, 1, 9, 5, 8)


@pytest.mark.parametrize("r", [0, 1, 2])
def test_head_on_swap(engine, r):
    spec, start, goal = swap_case()
    dev, _ = both(engine, spec, None, None, start, goal, 8, 2, r, 0, 10, 48)
    assert dev["status"].tolist() == [0, 0] and dev["arrive"].tolist() == [16, 16]
    assert dev["team_clearance"].tolist() == [r + 1] and dev["team_crossings"].tolist() == [0]


@pytest.mark.parametrize("r", [0, 1])
def test_lattice_team_of_16(engine, r):
    spec, start, goal = lattice_case()
    dev, _ = both(engine, spec, None, None, start, goal, 16, 16, r, 0, 10, 48)
    assert np.all(dev["status"] == R.PLANNED) and dev["team_clearance"][0] > r and dev["team_crossings"][0] == 0


def test_more_teams_than_workgroups(engine):
    """G = 64 and T = 256: a field is 257 x 64 x 64 x 4 bytes, so the 256 MiB cap on scratch allows 63 workgroups.  64 teams of 2:
    workgroup 0 takes team 0 and then team 63, on the scratch, stamps and walk cells team 0 left behind.  Teams do not see each
    other, so the rule on the robots of the teams 0, 1, 62 and 63 alone gives what the device must give for them."""
    spec = GridSpec(EXTENT, 64, INFLATE)
    rng = np.random.default_rng(4)
    start, goal = (rng.uniform(-1.8, 1.8, (128, 2)).astype(np.float32) for _ in range(2))
    goal[126], goal[127] = start[127], start[126]                                # the last team swaps places
    dev = engine.plan_grid_team(spec, None, None, teams=teams(2), reserve=1, start=start, goal=goal, layer_steps=10, layers=256, max_waypoints=8,
                                want_walks=True)
    assert dev["workgroups"] == 63 < 64 == len(dev["team_clearance"])
    rows = np.array([0, 1, 2, 3, 124, 125, 126, 127])
    ref = grid_plan_team(spec, None, None, start[rows], goal[rows], 8, teams(2), 1, 0, 10, 256, want_fields=False)
    for k in ("waypoints", "n_waypoints", "count", "status", "cost", "waits", "leave", "arrive", "release"):
        assert np.array_equal(dev[k][rows].view(np.uint32), ref[k].view(np.uint32)), k
    assert [dev["walks"][i] for i in rows] == ref["walks"]
    assert np.array_equal(dev["team_clearance"][[0, 1, 62, 63]], ref["team_clearance"]) and ref["team_clearance"][3] > 1
    assert not np.any(dev["status"] == R.UNCONVERGED)


def test_g128_two_layers_use_the_large_lds_path(engine):
    walls = Walls(SCENE0, radius=0.05)
    start = np.array([[-1.2, -1.2], [1.2, 1.2]], np.float32)
    both(engine, GridSpec(EXTENT, 128), walls, None, start, start[::-1].copy(), 12, 2, 2, 3, 20, 2)


def test_g64_serpentine_with_both_starts_on_it(engine):
    spec, walls, start, goal = serpentine()
    start2 = np.concatenate([start, start + np.array([[0.3, 0.0]], np.float32)])
    dev, ref = both(engine, spec, walls, None, start2, np.tile(goal, (2, 1)) + np.array([[0.0, 0.0], [-0.3, 0.0]], np.float32), 64, 2, 1, 0, 10, 4)
    print("serpentine sweeps:", dev["sweeps"], "arrive:", dev["arrive"], "status:", dev["status"])
    assert dev["sweeps"].max() > 2 * 64 and not np.any(dev["status"] == R.UNCONVERGED)
    assert dev["arrive"].max() + 1 > 4 + 1 + 2 * 64                               # longer than the walks' first buffer: the engine asked again


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
        got = eb.plan_grid_team(spec, walls, hz, teams=teams(4), reserve=1, start=start, goal=goal, step0=it, layer_steps=10, layers=8, max_waypoints=4)
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
    for change, word in ((dict(reserve=5), "reserve"), (dict(reserve=-1), "reserve"), (dict(layers=0), "layers"), (dict(layer_steps=0), "layer_steps"),
                         (dict(step0=-1), "step0"), (dict(max_waypoints=0), "max_waypoints"), (dict(start=start[:31], goal=goal[:31]), "do not split")):
        with pytest.raises(ValueError, match=word):
            engine.plan_grid_team(spec, walls if "start" not in change else None, hz if "start" not in change else None, **dict(kw, **change))
    with pytest.raises(ValueError, match="one scene"):
        engine.plan_grid_team(spec, two_scenes(np.arange(32) % 2), None, **kw)
    with pytest.raises(ValueError, match="exceed the cap"):
        engine.plan_grid_team(GridSpec(EXTENT, 128), None, None, teams=teams(2), reserve=1, start=np.zeros((64, 2), np.float32),
                              goal=np.zeros((64, 2), np.float32), layer_steps=1, layers=256, want_fields=True)


def test_c_entry_point_refusals_with_hand_made_structs(engine):
    """the checks of mobrob_ppo_plan_grid_team itself: PPOEngine.plan_grid_team refuses the same things before the call"""
    from mobrob_amd import _lib
    spec, walls, hz, start, goal = circling32()
    i32, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)

    def call(n=32, team_size=2, reserve=1, time=(0, 10, 8), scene=None, walk_cap=0, n_fields=None, null_time=False, **change):
        sp = _lib.PlanSpec()
        sp.n_robots, sp.pos_dim, sp.cells, sp.max_waypoints, sp.n_scenes, sp.n_fields = n, 2, 32, 4, 2, n if n_fields is None else n_fields
        sp.extent, sp.h, sp.inv_h, sp.inflate = float(spec.extent), float(spec.h), float(spec.inv_h), INFLATE
        for k, v in change.items():
            setattr(sp, k, v)
        tm = _lib.PlanTime()
        tm.step0, tm.layer_steps, tm.layers = time
        sc = np.ascontiguousarray(walls.scene[:n] if scene is None else scene, np.int32)
        wl = _lib.WallsC()
        wl.n_scenes, wl.max_walls = walls.n_scenes, walls.max_walls
        wl.boxes, wl.n_walls = walls.table.ctypes.data_as(fp), walls.counts.ctypes.data_as(i32)
        wl.scene, wl.radius, wl.cost, wl.indicator = sc.ctypes.data_as(i32), walls.radius, walls.cost, 1
        wp, rows, out = np.zeros((n, 4, 2), np.float32), [np.zeros((n, 4), np.int32) for _ in range(2)], [np.zeros(n, np.int32) for _ in range(5)]
        walk = np.zeros((n, max(walk_cap, 1)), np.uint16)
        return _lib.check(engine.lib.mobrob_ppo_plan_grid_team(
            engine._h, C.byref(sp), C.byref(wl), None, None if null_time else C.byref(tm), team_size, reserve, start.ctypes.data_as(fp),
            goal.ctypes.data_as(fp), wp.ctypes.data_as(fp), *(o.ctypes.data_as(i32) for o in out[:4]), *(o.ctypes.data_as(i32) for o in rows),
            out[4].ctypes.data_as(i32), None, walk.ctypes.data_as(C.POINTER(C.c_uint16)) if walk_cap else None, walk_cap, None, None, None))
    assert call() == 0 and call(walk_cap=5) == 0
    for args, word in ((dict(team_size=3), "team_size must be 1, 2, 4, 8 or 16"), (dict(team_size=32), "team_size must be 1, 2, 4, 8 or 16"),
                       (dict(team_size=0), "team_size"), (dict(n=31), "31 robots do not split into teams of 2"),
                       (dict(reserve=5), "reserve must lie in 0 .. 4"), (dict(reserve=-1), "reserve must lie in 0 .. 4"),
                       (dict(scene=np.arange(32) % 2), "one scene"), (dict(n_fields=16), "n_fields = 16 must be n_robots"),
                       (dict(time=(2 ** 31 - 90, 10, 8)), "fit an int32"), (dict(time=(0, 10, 0)), "layers must lie in 1 .. 256"),
                       (dict(time=(0, 10, 257)), "layers must lie in 1 .. 256"), (dict(time=(0, 0, 8)), "layer_steps"), (dict(time=(-1, 10, 8)), "step0"),
                       (dict(null_time=True), "null argument"), (dict(reuse_id=7), "reuse_id"), (dict(cells=48), "cells must be 32, 64 or 128"),
                       (dict(max_waypoints=0), "max_waypoints"), (dict(n_scenes=3), "n_scenes"), (dict(inflate=-1.0), "inflate")):
        with pytest.raises(ValueError, match=word):
            call(**args)
    assert call() == 0


def test_closed_loop_three_rounds_with_the_team_callback_on_the_device():
    """follow_with_replanning on the reference checkpoint's weights with teams= and the planner's team callback, device path"""
    e, _ = _engine("point", KW)
    e.set_params(golden_params(load_golden("point")))
    spec, start, goal = lattice_case()
    rng = np.random.default_rng(1)
    lat = np.stack(np.meshgrid(np.arange(32)[4:28:3], np.arange(32)[4:28:3]), axis=-1).reshape(-1, 2)
    cells = lat[rng.choice(len(lat), 64, replace=False)]
    start, goal = centres(spec, cells[:32]), centres(spec, cells[32:])
    tm, r = Teams(4, 0.1), 0
    env = _env("point", 32)
    planner = GridPlanner(env, engine=e, teams=tm, reserve=r, cells=32, inflate=INFLATE, max_waypoints=16, extent=EXTENT, layer_steps=5, layers=48)
    assert planner.device
    first = planner.plan(start, goal)
    host = grid_plan_team(spec, None, None, start, goal, 16, tm, r, 0, 5, 48, want_fields=False)
    same_time(first, host, ("waypoints", "n_waypoints", "count", "status", "cost", "waits", "leave", "arrive", "release", "team_clearance"))
    assert np.all(first["team_clearance"] > r)
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
        ref = grid_plan_team(spec, None, None, positions.astype(np.float32), goal, 16, tm, r, 20 * round_, 5, 48, want_fields=False)   # step0 = calls * horizon
        same_time(plan, ref, ("waypoints", "n_waypoints", "status", "release", "team_clearance"))
        replanned = sorted({i // 4 for i in new})
        print("round", round_, "replanned teams", replanned, "clearance", plan["team_clearance"][replanned], "conflict steps", out["conflict_steps"].sum())
        assert np.all(plan["team_clearance"][replanned] > r)
        for i, (w, rel) in new.items():
            assert plan["status"][i] == R.PLANNED and len(w) == plan["n_waypoints"][i] == len(rel)
    e.close()
