"""CPU: the grid planner's rule (goal_rules.GridSpec / grid_occupancy / grid_field / grid_path) and GridPlanner on the host path.

Everything the rule returns is an integer, a bool or a float32 produced by a fixed sequence of operations, so every comparison
here is exact.  The independent reference of grid_field is a synchronous Bellman-Ford over whole arrays (no heap, no order)."""
import numpy as np
import pytest

from mobrob_amd.envs import goal_rules as R
from mobrob_amd.envs.goal_rules import GridSpec, Hazards, MovingHazards, Walls, grid_field, grid_occupancy, grid_path, grid_plan, grid_walk
from mobrob_amd.planning import GridPlanner
from mobrob_amd.waypoints import FINISHED, GOING, STALLED

from tests.plan_scenes import EXTENT, INFLATE, POCKET, arena, robots33, serpentine, three_hazards, two_scenes

INF = 1 << 30


def bellman_ford(occ, goal_cell):
    """-> (field, sweeps): d <- min(d, shifted d + w) over all eight moves at once, until nothing changes"""
    G = occ.shape[0]
    free = np.zeros((G + 2, G + 2), bool)
    free[1:-1, 1:-1] = ~occ
    d = np.full((G + 2, G + 2), INF, np.int64)
    if free[1 + goal_cell // G, 1 + goal_cell % G]:
        d[1 + goal_cell // G, 1 + goal_cell % G] = 0
    core = (slice(1, -1), slice(1, -1))

    def shifted(a, dx, dy):
        return a[1 + dy:G + 1 + dy, 1 + dx:G + 1 + dx]
    sweeps = 0
    while True:
        sweeps += 1
        new = d[core].copy()
        for k, (dx, dy) in enumerate(R.PLAN_DIRS):
            ok = free[core] & shifted(free, dx, dy)
            if k >= 4:
                ok = ok & shifted(free, dx, 0) & shifted(free, 0, dy)
            new = np.where(ok, np.minimum(new, shifted(d, dx, dy) + (R.PLAN_STEP if k < 4 else R.PLAN_DIAG)), new)
        if np.array_equal(new, d[core]):
            break
        d[core] = new
    return np.where(d[core] >= INF, -1, d[core]).astype(np.int32), sweeps


@pytest.fixture(scope="module")
def scene32():
    scene, start, goal = robots33()
    spec, walls = GridSpec(EXTENT, 32, INFLATE), two_scenes(scene)
    return spec, walls, scene, start, goal, grid_plan(spec, walls, None, start, goal, 4)


def test_grid_numbers_are_the_float32_ones():
    spec = GridSpec(EXTENT, 32)
    assert spec.h == np.float32(0.125) and spec.inv_h == np.float32(8.0) and spec.h.dtype == np.float32
    assert spec.inflate_for(Walls(arena([]), radius=0.05)) == np.float32(np.float32(0.05) + np.float32(0.125))
    ix, iy = spec.cell_of(np.array([[-5.0, 5.0], [-2.0, 1.999], [0.0, -0.001]]))
    assert ix.tolist() == [0, 0, 16] and iy.tolist() == [31, 31, 15]
    assert spec.centre(0) == np.float32(-1.9375) and spec.centre(31) == np.float32(1.9375)
    odd = GridSpec(1.7, 64)   # h is not a power of two: every operation is a float32 one
    c = odd.centre(np.arange(64))
    assert c.dtype == np.float32 and np.array_equal(c, (-odd.extent + ((np.arange(64, dtype=np.float32) + np.float32(0.5)) * odd.h).astype(np.float32)))


def test_occupancy_equality_blocks_and_hazards_count(scene32):
    spec, walls, scene, *_ = scene32
    occ = grid_occupancy(spec, walls)
    assert occ.shape == (2, 32, 32) and occ.dtype == bool and occ[0].any() and not np.array_equal(occ[0], occ[1])
    # a box whose face is exactly `inflate` from a cell centre blocks that cell: centre 0.0625, face at 0.0625 + 0.25
    one = Walls([[0.5625, 0.0625, 0.25, 0.01]])
    for inflate, blocked in ((0.25, True), (np.nextafter(np.float32(0.25), np.float32(0)), False)):
        assert grid_occupancy(GridSpec(EXTENT, 32, inflate), one)[0, 16, 16] == blocked
    hz = Hazards([[0.0625, 0.3125]], size=0.125)                      # distance 0.25 from the centre (0.0625, 0.0625)
    assert grid_occupancy(GridSpec(EXTENT, 32, 0.125), None, hz)[0, 16, 16]
    assert not grid_occupancy(GridSpec(EXTENT, 32, 0.1249), None, hz)[0, 16, 16]
    both = grid_occupancy(spec, walls, three_hazards(scene))
    assert np.all(both >= occ) and both.sum() > occ.sum()
    assert not grid_occupancy(spec).any() and grid_occupancy(spec).shape == (1, 32, 32)


def test_field_is_bellman_ford_s_fixed_point(scene32):
    spec, walls, _, _, _, plan = scene32
    occ = plan["occupancy"]
    assert len(plan["field_goal_cell"]) == 14 and len(np.unique(plan["field_of"])) == 14      # 7 goals x 2 scenes, shared by 33 robots
    for f in range(14):
        ref, _ = bellman_ford(occ[plan["field_scene"][f]], int(plan["field_goal_cell"][f]))
        assert np.array_equal(plan["fields"][f], ref), f
        assert plan["fields"][f].dtype == np.int32
    hz_occ = grid_occupancy(spec, walls, three_hazards(walls.scene))
    for s in range(2):
        assert np.array_equal(grid_field(hz_occ[s], 5 * 32 + 5), bellman_ford(hz_occ[s], 5 * 32 + 5)[0])


def test_diagonal_between_two_boxes_is_not_taken():
    occ = np.zeros((32, 32), bool)
    occ[10, 10] = occ[11, 11] = True                                    # two boxes touching at a corner
    d = grid_field(occ, 10 * 32 + 11)                                   # goal (ix 11, iy 10); (ix 10, iy 11) is diagonal to it
    assert d[11, 10] > R.PLAN_DIAG and d[11, 10] == bellman_ford(occ, 10 * 32 + 11)[0][11, 10]
    assert d[9, 12] == R.PLAN_DIAG                                      # an open diagonal costs 7
    spec = GridSpec(EXTENT, 32, 0.0)
    cells, dirs, status = grid_walk(d, occ, spec, [spec.centre(10), spec.centre(11)], [spec.centre(11), spec.centre(10)])
    assert status == R.PLANNED and cells[0] == (10, 11) and cells[-1] == (11, 10) and len(cells) > 2
    one_free = occ.copy()
    one_free[11, 11] = False                                            # one blocked corner cell is enough to forbid the cut
    assert grid_field(one_free, 10 * 32 + 11)[11, 10] == 2 * R.PLAN_STEP


def test_sealed_goal_blocked_start_same_cell_and_truncation(scene32):
    spec, walls, scene, start, goal, plan = scene32
    occ, st, cnt, cost = plan["occupancy"], plan["status"], plan["count"], plan["cost"]
    assert set(st.tolist()) == {R.PLANNED, R.UNREACHABLE, R.TRUNCATED}
    # a goal in a blocked cell: an all -1 field, status 1
    f = grid_field(occ[0], int(np.flatnonzero(occ[0])[0]))
    assert np.all(f == -1)
    w, c, s, co = grid_path(f, occ[0], spec, [-1.2, -1.2], [1.2, 1.2], 4)
    assert (c, s, co) == (0, R.UNREACHABLE, -1) and not w.any()
    # blocked start cells (robots 0 and 1), the way out of the sealed pocket (robot 6), the way into it (robots 18 and 32)
    for i in (0, 1, 6, 18, 32):
        assert (st[i], cnt[i], cost[i], plan["n_waypoints"][i]) == (R.UNREACHABLE, 0, -1, 0) and not plan["waypoints"][i].any(), i
    # the sealed goal's field is finite inside the pocket only
    fp = plan["fields"][plan["field_of"][18]]
    inside = fp >= 0
    assert inside.any() and inside.sum() < 40 and fp[spec.cell_of(np.float32(POCKET))[::-1]] == 0
    # start cell = goal cell: the goal itself is the single waypoint (robots 2 and 3; robot 4 inside the pocket plans normally)
    for i in (2, 3):
        assert (st[i], cnt[i], cost[i]) == (R.PLANNED, 1, 0) and np.array_equal(plan["waypoints"][i, 0], goal[i])
    assert st[4] == R.PLANNED and cost[4] > 0
    # K too small: the count is the full path's, the first K waypoints are the full path's first K
    full = grid_plan(spec, walls, None, start, goal, int(cnt.max()), plan["occupancy"], plan["fields"])
    assert np.all(full["status"][st == R.TRUNCATED] == R.PLANNED) and np.array_equal(full["count"], cnt) and cnt.max() > 4
    assert np.array_equal(full["waypoints"][:, :4], plan["waypoints"]) and np.array_equal(plan["n_waypoints"], np.minimum(cnt, 4))
    for i in np.flatnonzero(st != R.UNREACHABLE):
        assert np.array_equal(full["waypoints"][i, cnt[i] - 1], goal[i]) and not full["waypoints"][i, cnt[i]:].any()


def test_every_step_of_a_path_obeys_the_move_rule_and_sums_to_the_cost(scene32):
    spec, walls, scene, start, goal, plan = scene32
    checked = 0
    for i in np.flatnonzero(plan["status"] != R.UNREACHABLE):
        f = plan["field_of"][i]
        occ, d = plan["occupancy"][plan["field_scene"][f]], plan["fields"][f]
        cells, dirs, _ = grid_walk(d, occ, spec, start[i], goal[i])
        total, turns = 0, 0
        for j, k in enumerate(dirs):
            (ix, iy), (jx, jy) = cells[j], cells[j + 1]
            assert (jx - ix, jy - iy) == R.PLAN_DIRS[k] and R.plan_move_ok(occ, ix, iy, k) and not occ[jy, jx]
            if k >= 4:
                assert not occ[iy, jx] and not occ[jy, ix]
            total += R.PLAN_STEP if k < 4 else R.PLAN_DIAG
            turns += j > 0 and dirs[j] != dirs[j - 1]
        assert total == plan["cost"][i] == d[cells[0][1], cells[0][0]] and turns + 1 == plan["count"][i]
        checked += len(dirs)
    assert checked > 100


def test_serpentine_needs_more_than_2G_sweeps():
    spec, walls, start, goal = serpentine()
    out = grid_plan(spec, walls, None, start, goal, 64)
    assert out["status"][0] == R.PLANNED and out["count"][0] > 2 * 14
    cells, dirs, _ = grid_walk(out["fields"][0], out["occupancy"][0], spec, start[0], goal[0])
    assert len(dirs) > 2 * spec.cells                  # a relaxation that moves one cell a sweep needs as many sweeps as moves
    ref, sweeps = bellman_ford(out["occupancy"][0], int(out["field_goal_cell"][0]))
    assert np.array_equal(ref, out["fields"][0]) and sweeps > 2 * spec.cells


def test_grid_planner_on_an_env_name_returns_the_rule(scene32):
    spec, walls, scene, start, goal, plan = scene32
    planner = GridPlanner("point", walls=walls, cells=32, inflate=INFLATE, max_waypoints=4, extent=EXTENT)
    got = planner.plan(start, goal, want_occupancy=True, want_fields=True)
    for k in ("waypoints", "n_waypoints", "count", "status", "cost", "occupancy", "fields", "field_of", "field_goal_cell", "field_scene"):
        assert np.array_equal(got[k], plan[k]) and got[k].dtype == plan[k].dtype, k
    assert got["waypoints"].view(np.uint32).tobytes() == plan["waypoints"].view(np.uint32).tobytes() and not got["fields_reused"]
    ok = plan["cost"] >= 0
    assert np.array_equal(got["cost_distance"][ok], plan["cost"][ok] * float(spec.h) / 5) and np.all(np.isnan(got["cost_distance"][~ok]))
    again = planner.plan(start[::-1].copy(), goal)             # the same goals: the fields are kept on the planner
    assert again["fields_reused"] and np.array_equal(again["cost"], grid_plan(spec, walls, None, start[::-1], goal, 4)["cost"])
    grown = planner.plan(start, goal, grow=True)
    assert grown["waypoints"].shape[1] == plan["count"].max() and not np.any(grown["status"] == R.TRUNCATED)
    assert np.array_equal(grown["count"], plan["count"])
    # the default inflate is the walls' radius + one cell; a drone's waypoints carry the goal's z
    assert GridPlanner("point", walls=walls, cells=32, extent=EXTENT).spec.inflate_for(walls) == np.float32(np.float32(0.05) + np.float32(0.125))
    g3 = np.concatenate([goal, np.full((33, 1), 0.7, np.float32)], axis=1)
    s3 = np.concatenate([start, np.zeros((33, 1), np.float32)], axis=1)
    d3 = GridPlanner("drone", walls=walls, cells=32, inflate=INFLATE, max_waypoints=4, extent=EXTENT).plan(s3, g3)
    assert np.array_equal(d3["waypoints"][:, :, :2], plan["waypoints"]) and np.array_equal(d3["status"], plan["status"])
    used = np.arange(4)[None, :] < d3["n_waypoints"][:, None]
    assert np.all(d3["waypoints"][:, :, 2][used] == np.float32(0.7)) and not d3["waypoints"][:, :, 2][~used].any()


def test_callback_plans_only_stalled_robots(scene32):
    spec, walls, scene, start, goal, plan = scene32
    planner = GridPlanner("point", walls=walls, cells=32, inflate=INFLATE, max_waypoints=8, extent=EXTENT)
    cb = planner.callback(goal)
    status = np.full(33, GOING)
    status[[3, 8]] = FINISHED
    assert cb(start, status, np.zeros(33, int)) == {} and cb.last is None
    status[[0, 6, 7, 9, 12]] = STALLED                           # 0 and 6 cannot be planned from where they stand
    new = cb(start, status, np.zeros(33, int))
    ref = grid_plan(spec, walls, None, start, goal, 8)
    assert sorted(new) == [7, 9, 12] and all(ref["status"][i] == R.PLANNED for i in new)
    for i, w in new.items():
        assert w.shape == (ref["count"][i], 2) and np.array_equal(w, ref["waypoints"][i, :ref["count"][i]])
    moved = start.copy()
    moved[12] = (-1.0, -1.0)
    second = cb(moved, status, np.zeros(33, int))
    assert cb.last["fields_reused"] and np.array_equal(second[12][-1], goal[12]) and not np.array_equal(second[12], new[12])


def test_refusals_name_the_argument(scene32):
    spec, walls, scene, start, goal, _ = scene32
    for bad, word in ((dict(cells=48), "cells"), (dict(cells=True), "cells"), (dict(extent=0.0), "extent"), (dict(extent=np.inf), "extent"),
                      (dict(inflate=-0.1), "inflate"), (dict(inflate=np.nan), "inflate")):
        kw = dict(extent=EXTENT, cells=32, inflate=None)
        kw.update(bad)
        with pytest.raises(ValueError, match=word):
            GridSpec(**kw)
    with pytest.raises(ValueError, match="agree on the scene"):
        grid_occupancy(spec, walls, three_hazards((scene + 1) % 2))
    with pytest.raises(ValueError, match="scenes"):
        grid_occupancy(spec, walls, Hazards([[0.0, 0.0]]))
    with pytest.raises(TypeError, match="moving hazards"):
        grid_occupancy(spec, None, MovingHazards(np.zeros((2, 1, 2))))
    with pytest.raises(ValueError, match="max_waypoints"):
        grid_path(np.zeros((32, 32), np.int32), np.zeros((32, 32), bool), spec, [0, 0], [0, 0], 0)
    with pytest.raises(ValueError, match="goal cell"):
        grid_field(np.zeros((32, 32), bool), 32 * 32)
    planner = GridPlanner("point", walls=walls, cells=32, extent=EXTENT)
    with pytest.raises(ValueError, match="start and goal"):
        planner.plan(start[:5], goal)
    with pytest.raises(ValueError, match="finite"):
        planner.plan(np.where(np.arange(33)[:, None] == 4, np.nan, start), goal)
    with pytest.raises(ValueError, match="wall scene must have 8 entries"):
        planner.plan(start[:8], goal[:8])
    with pytest.raises(ValueError, match="max_waypoints"):
        GridPlanner("point", max_waypoints=0)
    with pytest.raises(TypeError, match="env must be"):
        GridPlanner(object())


class _Wander:
    """a policy that needs no checkpoint: a fixed action"""

    def predict(self, obs, deterministic=True):
        return np.array([0.6, 0.3]), None


def test_cli_plans_to_a_goal(capsys):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("follow_cli", os.path.join(root, "examples", "follow.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    box = np.array([[0.0, 0.0, 0.05, 0.6]])
    r = cli.follow("point", "ppo", None, 4, max_steps=30, host=True, seed=3, policy=_Wander(), walls=box, arena=True, goal=[0.7, 0.7],
                   plan_cells=64, horizon=10, leg_steps=4)
    out = capsys.readouterr().out.splitlines()
    assert out[0].startswith("planned rate: ") and float(out[0].split(": ")[1]) >= 0.5 and out[1].startswith("success rate: ") and any(ln.startswith("stalled rate: ") for ln in out)
    nw = r["state"].n_waypoints
    assert np.sum(nw >= 1) >= 2 and all(np.array_equal(r["state"].waypoints[i, nw[i] - 1], np.float32([0.7, 0.7])) for i in range(4) if nw[i])
    with pytest.raises(ValueError, match="not both"):
        cli.follow("point", "ppo", np.zeros((1, 2)), 4, host=True, policy=_Wander(), goal=[1.0, 1.0])
    with pytest.raises(ValueError, match="not both"):
        cli.follow("point", "ppo", None, 4, host=True, policy=_Wander())
    with pytest.raises(ValueError, match="--goal must hold 2"):
        cli.follow("point", "ppo", None, 4, host=True, policy=_Wander(), goal=[1.0, 1.0, 1.0])
