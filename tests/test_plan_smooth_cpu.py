"""CPU: the line-of-sight smoothing rule of the grid planner (goal_rules.grid_los, grid_smooth, grid_path_smooth, grid_plan(smooth=)),
GridPlanner on the host path, the new symbol and the CLI flags.  All integers: nothing here has a tolerance.

What holds for which margin.  At margin 0 a straight run of the walk is always visible from its first cell (an orthogonal run
visits free cells, a diagonal move has both corner cells free by plan_move_ok), so between two emitted cells lies a change of
direction and count <= the unsmoothed count for every robot.  At margin 1 a cell next to a blocked cell is not clear: a walk ALONG
blocked cells sees nothing and keeps every cell (robots33 at G = 32 with walls: 134 waypoints against 62 unsmoothed, 42 at margin
0), so that bound is asserted at margin 0 and on scenes without blocked cells only; every leg passing grid_los, ascending indices
and the untouched robots are asserted at both margins."""
import importlib.util
import os

import numpy as np
import pytest

from mobrob_amd.envs import goal_rules as R
from mobrob_amd.envs.goal_rules import GridSpec, grid_los, grid_plan, grid_smooth
from mobrob_amd.planning import GridPlanner
from mobrob_amd.waypoints import FINISHED, GOING, STALLED
from tests.plan_scenes import EXTENT, INFLATE, robots33, serpentine, two_scenes
from tests.plan_smooth_cases import KEYS, corners_met, same_plan, walks, window_edges


def grid(rows):
    """an occupancy from rows of '.' and '#', the first row is iy = 0"""
    return np.array([[ch == "#" for ch in row] for row in rows], bool)


def test_los_on_hand_written_occupancies():
    free = np.zeros((8, 8), bool)
    assert grid_los(free, (0, 0), (7, 0)) and grid_los(free, (0, 0), (7, 3)) and grid_los(free, (2, 6), (2, 6)) and grid_los(free, (7, 7), (0, 1), 1)
    one = free.copy()
    one[0, 4] = True                                                # cell (4, 0)
    assert not grid_los(one, (0, 0), (7, 0)) and not grid_los(one, (7, 0), (0, 0)) and grid_los(one, (0, 1), (7, 1))
    assert not grid_los(one, (4, 0), (4, 3)) and not grid_los(one, (4, 3), (4, 0))          # an end cell that is blocked
    assert not grid_los(one, (0, 0), (7, 1))                        # the supercover of a shallow line visits (4, 0) ...
    assert grid_los(one, (0, 1), (7, 2))                            # ... and this one does not
    # exactly through the corner shared by (0,0), (1,0), (0,1), (1,1)
    assert grid_los(free, (0, 0), (2, 2))
    for cell in ((1, 0), (0, 1)):
        cut = free.copy()
        cut[cell[1], cell[0]] = True
        assert not grid_los(cut, (0, 0), (2, 2)) and not grid_los(cut, (2, 2), (0, 0)), cell
    far = free.copy()
    far[0, 2] = True                                                # (2, 0) shares no corner the segment passes
    assert grid_los(far, (0, 0), (2, 2))
    assert R.los_walk(free, (0, 0), (2, 2)) == (True, 2, 2) and R.los_walk(free, (0, 0), (4, 1))[2] == 0


def test_los_margin_1_next_to_a_blocked_cell_and_at_the_grid_edge():
    occ = np.zeros((8, 8), bool)
    occ[3, 3] = True
    assert grid_los(occ, (0, 1), (7, 1), 0) and grid_los(occ, (0, 1), (7, 1), 1)            # two cells away: clear
    assert grid_los(occ, (0, 2), (7, 2), 0) and not grid_los(occ, (0, 2), (7, 2), 1)        # passes next to the blocked cell
    assert grid_los(occ, (4, 4), (7, 7), 0) and not grid_los(occ, (4, 4), (7, 7), 1)        # the diagonal neighbour is not clear
    assert grid_los(occ, (5, 5), (7, 7), 1)
    assert np.array_equal(R.grid_dilate(occ), grid(["........", "........", "..###...", "..###...", "..###...", "........", "........", "........"]))
    # cells outside the grid count as free: the border row is clear at margin 1
    assert grid_los(np.zeros((8, 8), bool), (0, 0), (7, 0), 1) and grid_los(np.zeros((8, 8), bool), (0, 0), (0, 7), 1)
    edge = np.zeros((8, 8), bool)
    edge[1, 7] = True
    assert not grid_los(edge, (0, 0), (7, 0), 1) and grid_los(edge, (0, 0), (5, 0), 1) and not grid_los(edge, (0, 0), (6, 0), 1)
    assert R.grid_dilate(edge).sum() == 6
    for bad in (2, -1, True, 0.5):
        with pytest.raises(ValueError, match="margin"):
            grid_los(occ, (0, 0), (1, 1), bad)


def test_los_is_symmetric_and_takes_at_most_dx_plus_dy_steps():
    rng = np.random.default_rng(4)
    occ = rng.random((16, 16)) < 0.12
    seen = hidden = 0
    for margin in (0, 1):
        blk = R.los_blocked(occ, margin)
        for a in range(256):
            for b in range(a, 256):
                ca, cb = (a % 16, a // 16), (b % 16, b // 16)
                ab, steps, _ = R.los_walk(blk, ca, cb)
                ba, back, _ = R.los_walk(blk, cb, ca)
                assert ab == ba, (margin, ca, cb)
                assert max(steps, back) <= abs(ca[0] - cb[0]) + abs(ca[1] - cb[1])
                seen, hidden = seen + ab, hidden + (not ab)
    assert seen > 1000 and hidden > 1000


@pytest.fixture(scope="module")
def cases():
    """(name, spec, walls, start, goal, unsmoothed rule plan) of robots33 at G = 32, the serpentine at G = 64 and an empty grid"""
    scene, start, goal = robots33()
    walls = two_scenes(scene)
    spec = GridSpec(EXTENT, 32, INFLATE)
    out = [("robots33", spec, walls, start, goal, grid_plan(spec, walls, None, start, goal, 64))]
    sspec, swalls, sstart, sgoal = serpentine()
    out.append(("serpentine", sspec, swalls, sstart, sgoal, grid_plan(sspec, swalls, None, sstart, sgoal, 64)))
    espec = GridSpec(EXTENT, 32)
    out.append(("empty", espec, None, start, goal, grid_plan(espec, None, None, start, goal, 64)))
    return out


@pytest.mark.parametrize("margin", [0, 1])
def test_smooth_on_the_plan_scenes(cases, margin):
    for name, spec, walls, start, goal, plan in cases:
        sm = grid_plan(spec, walls, None, start, goal, 700, plan["occupancy"], plan["fields"], smooth=True, margin=margin)   # K: no truncation
        assert np.array_equal(sm["cost"], plan["cost"]) and np.array_equal(sm["status"] == R.UNREACHABLE, plan["status"] == R.UNREACHABLE)
        legs = 0
        for i, cells in enumerate(walks(plan, spec, start, goal)):
            occ = plan["occupancy"][plan["field_scene"][plan["field_of"][i]]]
            if not cells:                                           # unreachable: unchanged
                assert sm["count"][i] == plan["count"][i] == 0 and sm["moves"][i] == 0 and not sm["waypoints"][i].any()
                continue
            assert sm["moves"][i] == len(cells) - 1
            if len(cells) == 1:                                     # a start in the goal's cell: the goal alone
                assert sm["count"][i] == plan["count"][i] == 1 and np.array_equal(sm["waypoints"][i, :64], plan["waypoints"][i])
            keep = grid_smooth(cells, occ, margin)
            assert keep == sorted(set(keep)) and all(0 < j < len(cells) - 1 for j in keep) and sm["count"][i] == len(keep) + 1
            ends = [0] + keep + [len(cells) - 1]
            for u, v in zip(ends[:-1], ends[1:]):
                if v - u >= 2:
                    assert grid_los(occ, cells[u], cells[v], margin), (name, i, u, v)
                    legs += 1
            for slot, j in enumerate(keep):                         # every emitted cell lies on the walk: its centre is the waypoint
                assert np.array_equal(sm["waypoints"][i, slot], np.float32([spec.centre(cells[j][0]), spec.centre(cells[j][1])]))
            assert np.array_equal(sm["waypoints"][i, len(keep)], goal[i]) and not sm["waypoints"][i, len(keep) + 1:].any()
        assert legs > 0 or (name == "serpentine" and margin == 1)   # (its lanes hold no clear cell at margin 1: every cell is kept)
        print(f"{name} margin {margin}: {plan['count'].sum()} waypoints unsmoothed, {sm['count'].sum()} smoothed")
        if margin == 0 or name == "empty":                          # (the module docstring: why not margin 1 beside blocked cells)
            assert np.all(sm["count"] <= plan["count"]), name
        if name == "robots33" and margin == 0:
            assert sm["count"].sum() < plan["count"].sum()
        if name == "empty":
            planned = plan["status"] == R.PLANNED
            assert planned.all() and np.all(sm["count"] == 1) and sm["count"].sum() < plan["count"].sum()
        if name == "serpentine":
            assert sm["moves"][0] == 656 and (sm["count"][0] < plan["count"][0] if margin == 0 else True)


def test_window_edge_walks_have_the_lengths_they_are_named_for():
    spec, walls, start, goal, want = window_edges()
    sm = grid_plan(spec, walls, None, start, goal, 16, smooth=True, margin=0)
    assert np.array_equal(sm["moves"], want) and np.all(sm["status"] == R.PLANNED)
    assert np.all(sm["count"][:3] == 1) and np.all(sm["count"][3:] > 1)    # straight down the open half; around the bar


def test_smooth_false_reproduces_the_unsmoothed_plan(cases):
    name, spec, walls, start, goal, _ = cases[0]
    old = grid_plan(spec, walls, None, start, goal, 4)
    new = grid_plan(spec, walls, None, start, goal, 4, smooth=False, margin=0)
    assert sorted(old) == sorted(new) and "moves" not in new
    for k in old:
        assert old[k].dtype == new[k].dtype and np.array_equal(old[k], new[k]), k
    for i in range(len(start)):                                     # and grid_path itself, robot by robot
        f = old["field_of"][i]
        w, count, status, cost = R.grid_path(old["fields"][f], old["occupancy"][old["field_scene"][f]], spec, start[i], goal[i], 4)
        assert (count, status, cost) == (old["count"][i], old["status"][i], old["cost"][i]) and np.array_equal(w, old["waypoints"][i])
    assert corners_met(old, spec, start, goal, 0) > 0               # the scenes exercise the corner branch of the rule


def test_grid_planner_on_an_env_name_smooths(cases):
    _, spec, walls, start, goal, _ = cases[0]
    raw2 = grid_plan(spec, walls, None, start, goal, 2)
    sm2 = grid_plan(spec, walls, None, start, goal, 2, smooth=True, margin=0)
    gain = np.flatnonzero((raw2["status"] == R.TRUNCATED) & (sm2["status"] == R.PLANNED))
    assert gain.size > 0, "robots33 must hold a robot whose K = 2 plan is truncated unsmoothed and planned smoothed"
    planner = GridPlanner("point", walls=walls, cells=32, inflate=INFLATE, max_waypoints=2, extent=EXTENT, smooth=True, los_margin=0)
    got = planner.plan(start, goal)
    same_plan(got, sm2)
    assert got["smoothed"] and np.all(got["status"][gain] == R.PLANNED) and not got["fields_reused"]
    plain = planner.plan(start, goal, smooth=False)                 # the per-call override; today's bits, on the kept fields
    same_plan(plain, raw2, KEYS[:-1])
    assert not plain["smoothed"] and plain["moves"] is None and plain["fields_reused"] and np.all(plain["status"][gain] == R.TRUNCATED)
    # grow: the smoothed count sizes the second call
    assert np.any(sm2["status"] == R.TRUNCATED)
    grown = planner.plan(start, goal, grow=True)
    assert grown["waypoints"].shape[1] == sm2["count"].max() < raw2["count"].max() and not np.any(grown["status"] == R.TRUNCATED)
    same_plan(grown, grid_plan(spec, walls, None, start, goal, int(sm2["count"].max()), smooth=True, margin=0))
    # a planner that does not smooth can be asked to, with its own margin (default 1)
    other = GridPlanner("point", walls=walls, cells=32, inflate=INFLATE, max_waypoints=2, extent=EXTENT)
    assert other.los_margin == 1 and not other.plan(start, goal)["smoothed"]
    same_plan(other.plan(start, goal, smooth=True), grid_plan(spec, walls, None, start, goal, 2, smooth=True, margin=1))
    with pytest.raises(ValueError, match="los_margin"):
        GridPlanner("point", los_margin=2)


def test_callback_returns_smoothed_rows(cases):
    _, spec, walls, start, goal, _ = cases[0]
    planner = GridPlanner("point", walls=walls, cells=32, inflate=INFLATE, max_waypoints=8, extent=EXTENT, smooth=True, los_margin=0)
    cb = planner.callback(goal)
    status = np.full(33, GOING)
    status[[3, 8]] = FINISHED
    status[[0, 6, 7, 9, 12]] = STALLED
    new = cb(start, status, np.zeros(33, int))
    ref = grid_plan(spec, walls, None, start, goal, 8, smooth=True, margin=0)
    raw = grid_plan(spec, walls, None, start, goal, 8)
    assert sorted(new) == [7, 9, 12] and cb.last["smoothed"]
    for i, w in new.items():
        assert w.shape == (ref["count"][i], 2) and np.array_equal(w, ref["waypoints"][i, :ref["count"][i]])
    assert sum(len(w) for w in new.values()) < sum(int(raw["count"][i]) for i in new)


def test_symbol_and_cli_flags():
    from mobrob_amd import _lib
    assert "mobrob_ppo_plan_smooth" in _lib.SYMBOLS and len(_lib.SYMBOLS["mobrob_ppo_plan_smooth"][1]) == 13
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mobrob_ppo.h")).read()
    assert "int mobrob_ppo_plan_smooth(" in header
    spec = importlib.util.spec_from_file_location("follow_cli_smooth", os.path.join(root, "examples", "follow.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    ap = cli.build_parser()
    args = ap.parse_args(["--goal", "0.5,0.5", "--plan-smooth", "--plan-los-margin", "0"])
    assert args.plan_smooth is True and args.plan_los_margin == 0
    args = ap.parse_args(["--goal", "0.5,0.5"])
    assert args.plan_smooth is False and args.plan_los_margin == 1
    with pytest.raises(SystemExit):
        ap.parse_args(["--goal", "0.5,0.5", "--plan-los-margin", "2"])


class _Wander:
    def predict(self, obs, deterministic=True):
        return np.array([0.6, 0.3]), None


def test_cli_plans_smoothed(capsys):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("follow_cli_smooth2", os.path.join(root, "examples", "follow.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    box = np.array([[0.0, 0.0, 0.05, 0.6]])
    r = cli.follow("point", "ppo", None, 4, max_steps=20, host=True, seed=3, policy=_Wander(), walls=box, arena=True, goal=[0.7, 0.7],
                   plan_cells=64, plan_smooth=True, plan_los_margin=0)
    out = capsys.readouterr().out.splitlines()
    assert out[0].startswith("planned rate: ") and out[1].startswith("smoothed plan: ")
    nw = r["state"].n_waypoints
    assert all(np.array_equal(r["state"].waypoints[i, nw[i] - 1], np.float32([0.7, 0.7])) for i in range(4) if nw[i])
