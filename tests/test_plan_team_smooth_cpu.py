"""CPU: smoothing of a team plan, the NumPy rule against itself (goal_rules.grid_leg_cells, grid_smooth_time(max_leg),
grid_reserve_legs, grid_team_clearance_legs, grid_plan_team(smooth=True)), the planner's host path and every refusal by name.
Nothing here has a tolerance."""
import numpy as np
import pytest

from mobrob_amd.envs import goal_rules as R
from mobrob_amd.envs.goal_rules import grid_leg_cells, grid_plan_team, grid_plan_time, grid_reserve, grid_reserve_legs, los_walk
from mobrob_amd.planning import GridPlanner
from tests.plan_scenes import EXTENT, INFLATE
from tests.plan_team_scenes import circling32, lattice_case, swap_case, teams
from tests.plan_team_smooth_cases import brute_clearance, rule, rule_scenes

SCENES = rule_scenes()
SMOOTH = ("waypoints", "n_waypoints", "count", "status", "cost", "waits", "leave", "arrive", "release", "moves")


@pytest.mark.parametrize("name", sorted(SCENES))
def test_guarantee_by_brute_force_from_leg_cells_alone(name):
    """every pair of mates with walks is > reserve apart in every layer, the smallest distance is team_clearance, and a later member
    with a walk keeps > reserve from an earlier parked mate's start cell"""
    case = SCENES[name]
    size, T = case[5], case[7]
    for reserve in (0, 1, 2):
        for margin in (0, 1):
            for max_leg in (None, 8, 4):
                plan = rule(case, 8, reserve, margin, max_leg, want_fields=False)
                both, parked, pairs = brute_clearance(plan, size, T)
                # (the uncapped swap has no pair: member 0's one leg covers member 1's start cell, test_the_swap_needs_the_cap)
                assert pairs >= 1 or (name == "swap" and max_leg is None), (name, reserve, margin, max_leg)
                assert np.all(both > reserve) and np.all(parked > reserve), (name, reserve, margin, max_leg, both, parked)
                assert np.array_equal(plan["team_clearance"], both.astype(np.int32)), (name, reserve, margin, max_leg)
                for i, (w, k) in enumerate(zip(plan["walks"], plan["keeps"])):
                    assert len(w) == plan["arrive"][i] + 1 and k == sorted(set(k)) and all(0 < j < len(w) - 1 for j in k)
                    assert plan["count"][i] == (len(k) + 1 if plan["status"][i] != R.UNREACHABLE else 0)
                    legs = np.diff([0] + k + [len(w) - 1])
                    assert max_leg is None or np.all(legs <= max_leg)


@pytest.mark.parametrize("name", ["circling32_4", "lattice"])
def test_cap_one_is_the_unsmoothed_plan(name):
    spec, walls, hz, start, goal, size, layer_steps, layers = SCENES[name]
    for reserve in (0, 2):
        plain = grid_plan_team(spec, walls, hz, start, goal, 64, teams(size), reserve, 0, layer_steps, layers)
        capped = rule(SCENES[name], 64, reserve, 1, 1)
        for k in ("fields", "status", "cost", "arrive"):
            assert np.array_equal(plain[k], capped[k]), k
        assert plain["walks"] == capped["walks"]
        assert [list(range(1, len(w) - 1)) if s == R.PLANNED else [] for w, s in zip(capped["walks"], capped["status"])] == capped["keeps"]
        for w, k in zip(capped["walks"], capped["keeps"]):                          # the reservation is grid_reserve's
            assert np.array_equal(grid_reserve_legs(w, k, layers, spec.cells, reserve), grid_reserve(w, layers, spec.cells, reserve))


def size_one_rows(spec, ref, scene, goal, layers):
    """the robots that meet the size-1 condition of test_plan_team_cpu: no layer blocks a goal cell that an earlier layer left free"""
    gx, gy = spec.cell_of(goal)
    col = ref["occupancy"][scene, :, gy, gx]
    return np.array([not any(not col[i, t] and col[i, t + 1:].any() for t in range(layers)) for i in range(len(goal))])


@pytest.mark.parametrize("margin", [0, 1])
def test_size_one_and_every_first_member_equal_the_smoothed_time_plan(margin):
    spec, walls, hz, start, goal = circling32()
    scene = np.arange(32) // 16
    ref = grid_plan_time(spec, walls, hz, start, goal, 6, 0, 10, 8, smooth=True, margin=margin)
    rows = size_one_rows(spec, ref, scene, goal, 8)
    assert rows.sum() > 16, rows.sum()
    out = grid_plan_team(spec, walls, hz, start, goal, 6, teams(1), 2, 0, 10, 8, smooth=True, margin=margin, max_leg=None)
    for k in SMOOTH:
        assert np.array_equal(out[k][rows].view(np.uint32), ref[k][rows].view(np.uint32)), k
    assert np.array_equal(out["fields"][rows], ref["fields"][ref["field_of"]][rows]) and np.all(out["team_clearance"] == R.PLAN_NO_PAIR)
    four = grid_plan_team(spec, walls, hz, start, goal, 6, teams(4), 1, 0, 10, 8, smooth=True, margin=margin, max_leg=None)
    first = rows & (np.arange(32) % 4 == 0)
    assert first.sum() > 4, first.sum()
    for k in SMOOTH:
        assert np.array_equal(four[k][first].view(np.uint32), ref[k][first].view(np.uint32)), k


@pytest.mark.parametrize("reserve", [0, 1, 2])
def test_the_swap_needs_the_cap(reserve):
    spec, start, goal = swap_case()
    free = grid_plan_team(spec, None, None, start, goal, 8, teams(2), reserve, 0, 5, 48, smooth=True, margin=0, max_leg=None)
    assert free["status"].tolist() == [R.PLANNED, R.UNREACHABLE] and free["keeps"] == [[], []] and free["count"].tolist() == [1, 0]
    assert free["team_clearance"].tolist() == [R.PLAN_NO_PAIR]                      # one leg of 16 actions covers the mate's start cell
    capped = grid_plan_team(spec, None, None, start, goal, 8, teams(2), reserve, 0, 5, 48, smooth=True, margin=0, max_leg=8)
    assert capped["status"].tolist() == [R.PLANNED, R.PLANNED] and capped["team_clearance"].tolist() == [reserve + 1]
    plain = grid_plan_team(spec, None, None, start, goal, 8, teams(2), reserve, 0, 5, 48)
    assert capped["count"].sum() == plain["count"].sum() == 5
    assert np.array_equal(capped["release"], R.grid_release_smooth(capped["leave"], 0, 5)) and not np.any(capped["waits"])


class _Recorder:
    def __init__(self):
        self.seen = []

    def __getitem__(self, yx):
        self.seen.append((int(yx[1]), int(yx[0])))
        return False


def test_leg_cells_are_the_cells_the_sight_line_reads():
    assert grid_leg_cells((3, 3), (3, 3)) == [(3, 3)]
    assert set(grid_leg_cells((3, 3), (4, 4))) == {(3, 3), (4, 4), (4, 3), (3, 4)}   # a diagonal neighbour: both corner cells
    assert set(grid_leg_cells((3, 3), (2, 4))) == {(3, 3), (2, 4), (2, 3), (3, 4)}
    assert grid_leg_cells((3, 3), (4, 3)) == [(3, 3), (4, 3)] and grid_leg_cells((1, 0), (1, 3)) == [(1, 0), (1, 1), (1, 2), (1, 3)]
    cells = [(x, y) for y in range(12) for x in range(12)]
    for a in cells:
        for b in cells:
            rec = _Recorder()
            assert los_walk(rec, a, b)[0]
            got = grid_leg_cells(a, b)
            assert set(got) == set(rec.seen) and got[0] == a and got[-1] == b, (a, b)
            assert set(got) == set(grid_leg_cells(b, a)), (a, b)
            assert all(min(a[0], b[0]) <= x <= max(a[0], b[0]) and min(a[1], b[1]) <= y <= max(a[1], b[1]) for x, y in got)


def test_capped_smoothing_and_the_swept_reservation_on_a_hand_made_walk():
    nb = np.full((5, 12, 12), R.PLAN_NEVER_BLOCKED, np.int16)
    walk = [(x, 2) for x in range(8)] + [(7, 3), (7, 4)]                            # 9 actions: a row, then up
    assert R.grid_smooth_time(walk, nb) == [] and R.grid_smooth_time(walk, nb, None) == []
    assert R.grid_smooth_time(walk, nb, 4) == [4, 8] and R.grid_smooth_time(walk, nb, 1) == list(range(1, 9))
    assert R.grid_smooth_time(walk, nb, 9) == [] and R.grid_smooth_time(walk, nb, 8) == [8]
    res = grid_reserve_legs(walk, [4, 8], 6, 12, 0)                                  # legs (0, 4), (4, 8), (8, 9); T = 6 < A = 9
    row = {(x, 2) for x in range(5)}
    for t in range(4):
        assert {(int(x), int(y)) for y, x in zip(*np.nonzero(res[t]))} == row        # all of the leg in every layer of its span
    second = set(grid_leg_cells((4, 2), (7, 3)))
    assert {(int(x), int(y)) for y, x in zip(*np.nonzero(res[5]))} == second
    assert {(int(x), int(y)) for y, x in zip(*np.nonzero(res[6]))} == second | {(7, 3), (7, 4)}   # the tail: every leg from T on
    parked = grid_reserve_legs([(5, 5)], [], 3, 12, 1)
    assert parked.sum() == 4 * 9 and np.all(parked[:, 4:7, 4:7])
    assert R.grid_team_clearance_legs([walk, [(0, 4), (1, 4), (2, 4)]], [[4, 8], [1]], 2, 6).tolist() == [2]
    assert R.grid_team_clearance_legs([walk, [(0, 4), (1, 4), (2, 4)]], [[4, 8], None], 2, 6).tolist() == [R.PLAN_NO_PAIR]
    assert R.grid_team_clearance_legs([walk], [[4, 8]], 1, 6).tolist() == [R.PLAN_NO_PAIR]
    with pytest.raises(ValueError, match="do not split"):
        R.grid_team_clearance_legs([walk, walk, walk], [[], [], []], 2, 6)


def test_refusals_are_named():
    spec, start, goal = swap_case()
    kw = dict(smooth=True, margin=0)
    for bad in (0, -3, True, 2.0):
        with pytest.raises(ValueError, match="max_leg"):
            grid_plan_team(spec, None, None, start, goal, 8, teams(2), 1, 0, 5, 48, max_leg=bad, **kw)
    with pytest.raises(ValueError, match="max_leg"):
        R.grid_smooth_time([(0, 0), (1, 0), (2, 0)], np.zeros((2, 4, 4), np.int16), 0)
    for bad in (2, -1, True):
        with pytest.raises(ValueError, match="margin"):
            grid_plan_team(spec, None, None, start, goal, 8, teams(2), 1, 0, 5, 48, smooth=True, margin=bad)
    kwp = dict(cells=32, inflate=INFLATE, extent=EXTENT)
    with pytest.raises(ValueError, match="max_leg= belongs to teams"):
        GridPlanner("point", max_leg=8, **kwp)
    with pytest.raises(ValueError, match="max_leg= belongs to teams"):
        GridPlanner("point", hazards=circling32()[2], walls=circling32()[1], layer_steps=5, time_smooth=True, max_leg=None, **kwp)
    with pytest.raises(ValueError, match="max_leg"):
        GridPlanner("point", teams=teams(2), layer_steps=5, time_smooth=True, max_leg=0, **kwp)
    with pytest.raises(ValueError, match="los_margin"):
        GridPlanner("point", teams=teams(2), layer_steps=5, time_smooth=True, los_margin=2, **kwp)
    with pytest.raises(ValueError, match="time_smooth"):
        GridPlanner("point", teams=teams(2), layer_steps=5, smooth=True, **kwp)     # smooth= is the static smoother and still raises
    with pytest.raises(ValueError, match="time_smooth=True needs"):
        GridPlanner("point", time_smooth=True, **kwp)
    with pytest.raises(ValueError, match="teams of two or more"):                   # a team of one has no mates: refused as it always was
        GridPlanner("point", teams=teams(1), layer_steps=5, time_smooth=True, **kwp)
    with pytest.raises(ValueError, match="teams of two or more"):
        GridPlanner("point", teams=teams(1), layer_steps=5, **kwp).plan(np.zeros((1, 2)), np.ones((1, 2)), time_smooth=True)


def test_planner_host_path_smooths_a_team_plan_per_planner_and_per_call():
    spec, start, goal = lattice_case()
    kwp = dict(cells=32, inflate=INFLATE, extent=EXTENT, layer_steps=10, layers=48, max_waypoints=16)
    ref = grid_plan_team(spec, None, None, start, goal, 16, teams(16), 1, 0, 10, 48, smooth=True, margin=0, max_leg=4)
    planner = GridPlanner("point", teams=teams(16), reserve=1, time_smooth=True, los_margin=0, max_leg=4, **kwp)
    got = planner.plan(start, goal)
    for k in SMOOTH + ("team_clearance", "team_crossings"):
        assert np.array_equal(np.asarray(got[k]).view(np.uint32), np.asarray(ref[k]).view(np.uint32)), k
    assert got["smoothed"] and got["keeps"] == ref["keeps"] and np.all(got["team_clearance"] > 1)
    plain = GridPlanner("point", teams=teams(16), reserve=1, los_margin=0, **kwp)
    assert plain.max_leg == 8 and not plain.plan(start, goal)["smoothed"] and "keeps" not in plain.plan(start, goal)
    per_call = plain.plan(start, goal, time_smooth=True)
    ref8 = grid_plan_team(spec, None, None, start, goal, 16, teams(16), 1, 0, 10, 48, smooth=True, margin=0, max_leg=8)
    assert per_call["smoothed"] and per_call["keeps"] == ref8["keeps"] and np.array_equal(per_call["release"], ref8["release"])
    free = GridPlanner("point", teams=teams(16), reserve=1, time_smooth=True, los_margin=0, max_leg=None, **kwp)
    assert free.max_leg is None
    cb = planner.callback(goal, horizon=20)
    from mobrob_amd.waypoints import STALLED
    rows = cb(start, np.full(16, STALLED), np.zeros(16, bool))                        # planned again from where they stand
    assert cb.calls == 1 and rows
    again = grid_plan_team(spec, None, None, start, goal, 16, teams(16), 1, 20, 10, 48, smooth=True, margin=0, max_leg=4)
    for i, (w, rel) in rows.items():
        assert again["status"][i] == R.PLANNED and np.array_equal(w, again["waypoints"][i, :again["n_waypoints"][i]])
        assert np.array_equal(rel, again["release"][i, :len(w)])
