"""CPU: the clearance-aware grid plan by the NumPy rule (goal_rules.grid_clearance, grid_surcharge, grid_field_cost, grid_walk_cost,
grid_plan(..., clearance=)) and the GridPlanner host path.  All integers: nothing here has a tolerance."""
import numpy as np
import pytest

from mobrob_amd.envs import goal_rules as R
from mobrob_amd.envs.goal_rules import GridSpec, MovingHazards, Teams, Walls, grid_plan
from mobrob_amd.planning import GridPlanner
from tests.plan_scenes import EXTENT, INFLATE, robots33, two_scenes

G16 = 16


@pytest.fixture(scope="module")
def random16():
    """a random 16 x 16 map, a quarter of it blocked, and its brute-force Chebyshev distance to the nearest blocked cell"""
    rng = np.random.default_rng(41)
    occ = rng.random((G16, G16)) < 0.25
    by, bx = np.nonzero(occ)
    yy, xx = np.mgrid[:G16, :G16]
    dist = np.max(np.stack([np.abs(yy[..., None] - by), np.abs(xx[..., None] - bx)]), axis=0).min(axis=-1)
    return occ, dist


def test_clearance_and_surcharge_against_brute_force(random16):
    occ, dist = random16
    assert occ.any() and not occ.all()
    for reach in range(1, R.PLAN_CLEAR_REACH_MAX + 1):
        clear = R.grid_clearance(occ, reach)
        assert clear.dtype == np.uint8 and np.array_equal(clear, np.minimum(dist, reach + 1))
        assert np.all(clear[occ] == 0) and np.all(clear[~occ] >= 1)
        for weight in (1, 5, R.PLAN_CLEAR_WEIGHT_MAX):
            pen = R.grid_surcharge(occ, reach, weight)
            want = np.where(occ, 0, weight * np.maximum(0, reach + 1 - np.minimum(dist, reach + 1)))
            assert pen.dtype == np.uint8 and np.array_equal(pen, want) and pen.max() <= 128
    # an empty map: nothing within reach, cells outside the grid count as free
    assert np.all(R.grid_clearance(np.zeros((G16, G16), bool), 3) == 4) and not R.grid_surcharge(np.zeros((G16, G16), bool), 3, 7).any()
    assert R.grid_surcharge(~np.zeros((G16, G16), bool), 8, 16).max() == 0           # all blocked: no free cell pays
    one = np.zeros((G16, G16), bool)
    one[0, 0] = True
    assert R.grid_surcharge(one, 8, 16)[1, 1] == 128 and R.grid_surcharge(one, 8, 16)[0, 8] == 16 and R.grid_surcharge(one, 8, 16)[0, 9] == 0


def test_cost_field_is_the_fixed_point_and_the_walk_pays_it(random16):
    occ, _ = random16
    spec = GridSpec(1.0, 32)                                                          # only cell_of / centre are used: embed the map
    big = np.ones((32, 32), bool)
    big[:G16, :G16] = occ
    pen = R.grid_surcharge(big, 2, 5)
    free = np.flatnonzero(~big.ravel())
    fields = 0
    for goal_cell in free[[0, len(free) // 2, -1]]:
        d = R.grid_field_cost(big, pen, goal_cell)
        gy, gx = divmod(int(goal_cell), 32)
        assert d[gy, gx] == 0 and np.all(d[big] == -1)
        reachable = 0
        for c in free:
            iy, ix = divmod(int(c), 32)
            if (iy, ix) == (gy, gx):
                continue
            best = [(R.PLAN_STEP if k < 4 else R.PLAN_DIAG) + int(pen[iy + dy, ix + dx]) + int(d[iy + dy, ix + dx])
                    for k, (dx, dy) in enumerate(R.PLAN_DIRS) if R.plan_move_ok(big, ix, iy, k) and d[iy + dy, ix + dx] >= 0]
            assert d[iy, ix] == (min(best) if best else -1), (c, goal_cell)
            if d[iy, ix] < 0:
                continue
            reachable += 1
            start_xy, goal_xy = (spec.centre(ix), spec.centre(iy)), (spec.centre(gx), spec.centre(gy))
            cells, dirs, status = R.grid_walk_cost(d, big, pen, spec, start_xy, goal_xy)
            paid = sum((R.PLAN_STEP if k < 4 else R.PLAN_DIAG) + int(pen[y, x]) for k, (x, y) in zip(dirs, cells[1:]))
            _, _, st, cost = R.grid_path_cost(d, big, pen, spec, start_xy, goal_xy, 8)
            assert status == R.PLANNED and cells[0] == (ix, iy) and cells[-1] == (gx, gy) and paid == d[iy, ix] == cost and st in (0, 2)
        fields += reachable > 0
    assert fields >= 2, "the goals chosen must have cells that reach them"
    # with no surcharge the cost field is the plain field
    assert np.array_equal(R.grid_field_cost(big, np.zeros_like(pen), free[0]), R.grid_field(big, free[0]))


def test_neutral_on_an_empty_grid_and_none_is_todays_plan():
    spec = GridSpec(EXTENT, 32)
    rng = np.random.default_rng(3)
    start = rng.uniform(-1.0, 1.0, (6, 2)).astype(np.float32)                         # more than 2 cells from the border: |x| <= 1 < 2 - 3 h
    goal = rng.uniform(-1.0, 1.0, (6, 2)).astype(np.float32)
    for smooth in (False, True):
        plain = grid_plan(spec, None, None, start, goal, 4, smooth=smooth)
        clear = grid_plan(spec, None, None, start, goal, 4, smooth=smooth, clearance=(2, 4))
        assert not clear["surcharge"].any() and np.all(clear["clearance_min"] == 3)
        assert set(clear) - set(plain) == {"surcharge", "clearance_min"}
        for k in plain:
            assert clear[k].dtype == plain[k].dtype and clear[k].tobytes() == plain[k].tobytes(), k
    scene, s33, g33 = robots33()
    walls = two_scenes(scene)
    spec = GridSpec(EXTENT, 32, INFLATE)
    a, b = grid_plan(spec, walls, None, s33, g33, 4), grid_plan(spec, walls, None, s33, g33, 4, clearance=None)
    assert set(a) == set(b) and all(a[k].tobytes() == b[k].tobytes() and a[k].dtype == b[k].dtype for k in a)


ONE_BOX = np.array([[0.0, -0.3, 0.5, 0.55]])
BOX_START, BOX_GOAL = np.array([[-1.2, -0.9]], np.float32), np.array([[1.2, 0.6]], np.float32)


def test_the_point_of_it_room_is_taken_where_room_exists():
    """One box in open floor at 32 cells, the start below and left of it, the goal above and right.  By the rule alone:
    the plain plan rounds the box's corner at clearance 1 (cost 137, 25 moves) and its margin-1 smoothing keeps 5 waypoints;
    with clearance=(2, 8) the walk stays 3 cells away (the cap: no surcharged cell is entered; cost 150, 28 moves) and the margin-1
    smoothing keeps 2 waypoints."""
    spec, walls = GridSpec(EXTENT, 32, INFLATE), Walls(ONE_BOX, radius=0.05)
    plain = grid_plan(spec, walls, None, BOX_START, BOX_GOAL, 64, smooth=True, margin=1)
    clear = grid_plan(spec, walls, None, BOX_START, BOX_GOAL, 64, smooth=True, margin=1, clearance=(2, 8))
    plain_min = R.grid_plan_clearance_min(spec, plain, BOX_START, BOX_GOAL, 2)
    print("plain: clearance_min", plain_min, "count", plain["count"], "cost", plain["cost"], "moves", plain["moves"])
    print("clearance (2, 8): clearance_min", clear["clearance_min"], "count", clear["count"], "cost", clear["cost"], "moves", clear["moves"])
    assert plain["status"][0] == clear["status"][0] == R.PLANNED
    assert clear["clearance_min"][0] > plain_min[0]
    assert clear["count"][0] <= plain["count"][0]
    assert (plain_min[0], plain["count"][0], clear["clearance_min"][0], clear["count"][0]) == (1, 5, 3, 2)
    assert clear["cost"][0] >= plain["cost"][0] and clear["moves"][0] >= plain["moves"][0]     # no longer the shortest
    # the unsmoothed clearance plan walks the same cells
    walk = grid_plan(spec, walls, None, BOX_START, BOX_GOAL, 64, clearance=(2, 8))
    assert walk["clearance_min"][0] == 3 and walk["cost"][0] == clear["cost"][0]


@pytest.mark.parametrize("smooth", [False, True])
def test_grid_planner_host_path(smooth):
    scene, start, goal = robots33()
    walls = two_scenes(scene)
    planner = GridPlanner("point", walls=walls, cells=32, inflate=INFLATE, max_waypoints=4, extent=EXTENT, smooth=smooth, clearance=(2, 8))
    ref = grid_plan(planner.spec, walls, None, start, goal, 4, smooth=smooth, clearance=(2, 8))
    got = planner.plan(start, goal, want_occupancy=True, want_fields=True)
    for k in ("waypoints", "n_waypoints", "count", "status", "cost", "occupancy", "fields", "clearance_min"):
        assert got[k].dtype == ref[k].dtype and got[k].tobytes() == ref[k].tobytes(), k
    assert got["clearance"] == (2, 8) and got["smoothed"] == smooth and not got["fields_reused"]
    assert set(ref["status"].tolist()) >= {R.PLANNED, R.UNREACHABLE} and np.all((ref["clearance_min"] == -1) == (ref["status"] == R.UNREACHABLE))
    # a replanning round reuses the cost fields; a call without clearance does not, and returns today's plan
    moved = start[::-1].copy()
    again = planner.plan(moved, goal)
    assert again["fields_reused"]
    ref2 = grid_plan(planner.spec, walls, None, moved, goal, 4, smooth=smooth, clearance=(2, 8))
    assert again["waypoints"].tobytes() == ref2["waypoints"].tobytes() and np.array_equal(again["clearance_min"], ref2["clearance_min"])
    plain = planner.plan(moved, goal, clearance=None)
    ref3 = grid_plan(planner.spec, walls, None, moved, goal, 4, smooth=smooth)
    assert not plain["fields_reused"] and "clearance_min" not in plain
    assert plain["waypoints"].tobytes() == ref3["waypoints"].tobytes() and np.array_equal(plain["cost"], ref3["cost"])
    # grow and the callback plan with the planner's clearance
    grown = planner.plan(start, goal, grow=True)
    assert not np.any(grown["status"] == R.TRUNCATED) and grown["waypoints"].shape[1] == ref["count"].max()
    from mobrob_amd.waypoints import STALLED
    cb = planner.callback(goal)
    rows = cb(moved, np.full(33, STALLED), np.zeros(33, bool))
    assert cb.last["clearance"] == (2, 8) and sorted(rows) == [i for i in range(33) if ref2["status"][i] == R.PLANNED]


def test_the_two_new_symbols_are_declared_exported_and_bound():
    import ctypes
    import os
    import re
    from mobrob_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "mobrob_ppo.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in (("mobrob_ppo_plan_grid_clear", 22), ("mobrob_ppo_plan_smooth_clear", 14)):
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} is not declared in include/mobrob_ppo.h"
        assert hasattr(lib, name) and name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == n_args
    assert lib.mobrob_ppo_abi_version() == _lib.ABI_VERSION == 3
    planner_calls = sorted(n for n in _lib.SYMBOLS if n.startswith("mobrob_ppo_plan_"))
    assert len(planner_calls) == 10, planner_calls                                    # the eight before this feature and the two new ones


def test_every_new_refusal_names_clearance():
    for bad in ((0, 1), (9, 1), (1, 0), (1, 17), (True, 1), (1, True), (1.0, 1), (2,), 3, "ab"):
        with pytest.raises(ValueError, match="clearance"):
            R.plan_clearance_check(bad)
        with pytest.raises(ValueError, match="clearance"):
            GridPlanner("point", extent=EXTENT, clearance=bad)
    with pytest.raises(ValueError, match="clearance"):
        R.grid_clearance(np.zeros((32, 32), bool), True)
    with pytest.raises(ValueError, match="clearance"):
        grid_plan(GridSpec(EXTENT, 32), None, None, BOX_START, BOX_GOAL, 4, clearance=(1, 99))
    moving = MovingHazards.circling(np.array([[0.5, 0.5]]), travel=0.3, size=0.1, n_frames=4, dt=1.0, frame_steps=5, loop=True)
    teams = Teams(2, 0.3)
    for kw in (dict(hazards=moving, layer_steps=5), dict(teams=teams, layer_steps=5), dict(teams=teams, layer_steps=5, time_smooth=True),
               dict(hazards=moving, layer_steps=5, time_smooth=True), dict(teams=teams, layer_steps=5, assign="sum")):
        with pytest.raises(ValueError, match="clearance"):
            GridPlanner("point", extent=EXTENT, cells=32, clearance=(2, 8), **kw)
        planner = GridPlanner("point", extent=EXTENT, cells=32, **kw)
        with pytest.raises(ValueError, match="clearance"):
            planner.plan(np.zeros((2, 2)), np.ones((2, 2)), clearance=(2, 8))
    # the existing refusals stay what they were
    with pytest.raises(ValueError, match="retries"):
        GridPlanner("point", extent=EXTENT, cells=32, teams=teams, layer_steps=5, retries=1, time_smooth=True, clearance=(2, 8))


class _Wander:
    """a policy that needs no checkpoint: a fixed action"""

    def predict(self, obs, deterministic=True):
        return np.array([0.6, 0.3]), None


def test_cli_prints_the_clearance_plan_beside_the_plain_one(capsys):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("follow_cli", os.path.join(root, "examples", "follow.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    box = np.array([[0.0, 0.0, 0.05, 0.6]])
    kw = dict(max_steps=20, host=True, seed=3, policy=_Wander(), walls=box, arena=True, goal=[0.7, 0.7], plan_cells=64, plan_smooth=True)
    cli.follow("point", "ppo", None, 4, plan_clearance=[2, 8], **kw)
    out = capsys.readouterr().out.splitlines()
    line = [ln for ln in out if ln.startswith("clearance plan (2, 8): ")]
    assert len(line) == 1 and "least clearance" in line[0] and "without it: " in line[0] and any(ln.startswith("planned rate: ") for ln in out)
    with pytest.raises(ValueError, match="clearance"):
        cli.follow("point", "ppo", None, 4, plan_clearance=[9, 8], **kw)
    with pytest.raises(ValueError, match="clearance"):
        cli.follow("point", "ppo", None, 4, plan_clearance=[2, 8], team_size=2, **dict(kw, plan_smooth=False))   # (smooth= with teams is an older refusal)
