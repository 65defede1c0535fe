"""CPU: prioritised planning inside a team, the NumPy rule (goal_rules.grid_plan_team, grid_reserve, grid_team_field, grid_walk_team)
and its independent checker (grid_team_clearance), the planner's host path and every refusal by name.  Nothing here has a
tolerance."""
import numpy as np
import pytest

from mobrob_amd.envs import goal_rules as R
from mobrob_amd.envs.goal_rules import GridSpec, MovingHazards, Teams, grid_plan, grid_plan_team, grid_plan_time, grid_team_clearance
from mobrob_amd.planning import GridPlanner
from tests.plan_scenes import EXTENT, INFLATE, three_hazards, two_scenes
from tests.plan_team_scenes import (SPEC32, centres, circling32, crossing_goal_case, lattice_case, sealed_case, same_team, swap_case, teams)
from tests.plan_time_scenes import FAR, circling33, same_time

PLAN = ("waypoints", "n_waypoints", "count", "status", "cost")
TIME = PLAN + ("waits", "leave", "arrive", "release")


def alone_walks(spec, start, goal, T):
    """the walks of robots planned alone with grid_plan_time in an empty arena"""
    one = MovingHazards(np.array([[FAR]]))
    alone = grid_plan_time(spec, None, one, start, goal, 8, 0, 10, T)
    return [R.grid_walk_time(alone["fields"][alone["field_of"][i]], alone["occupancy"][0], spec, start[i], goal[i])[0] for i in range(len(start))]


@pytest.mark.parametrize("r", [0, 1, 2])
def test_head_on_swap_keeps_more_than_reserve_cells_where_plans_made_alone_collide(r):
    spec, start, goal = swap_case()
    out = grid_plan_team(spec, None, None, start, goal, 8, teams(2), r, 0, 10, 48)
    assert out["status"].tolist() == [R.PLANNED, R.PLANNED] and out["arrive"].tolist() == [16, 16]
    clear, cross = grid_team_clearance(out["walks"], 2, 48)
    assert clear.tolist() == [r + 1] and cross.tolist() == [0]
    assert np.array_equal(out["team_clearance"], clear) and np.array_equal(out["team_crossings"], cross)
    assert grid_team_clearance(alone_walks(spec, start, goal, 48), 2, 48)[0].tolist() == [0]     # what the feature is for


@pytest.mark.parametrize("r", [0, 1])
def test_lattice_team_of_16_all_planned_and_every_pair_checked(r):
    spec, start, goal = lattice_case()
    out = grid_plan_team(spec, None, None, start, goal, 16, teams(16), r, 0, 10, 48)
    assert np.all(out["status"] == R.PLANNED) and len(out["walks"]) == 16
    clear, cross = grid_team_clearance(out["walks"], 16, 48)
    assert clear[0] > r and cross[0] == 0
    for i, w in enumerate(out["walks"]):                                          # no robot is left out: every walk is its robot's
        assert len(w) == out["arrive"][i] + 1
        assert w[0] == tuple(int(v) for v in spec.cell_of(start[i])) and w[-1] == tuple(int(v) for v in spec.cell_of(goal[i]))
    worst = min(int(np.abs(np.array(out["walks"][i][min(t, len(out["walks"][i]) - 1)]) - np.array(out["walks"][j][min(t, len(out["walks"][j]) - 1)])).max())
                for i in range(16) for j in range(i + 1, 16) for t in range(49))
    assert worst >= clear[0]                                                      # a plain in-step recount never undercuts the checker


def test_the_checker_counts_crossings_and_tails_and_sees_walks_only():
    a, b = [(0, 0), (1, 1)], [(1, 0), (0, 1)]                                       # the two diagonals of one block, in one action
    assert [v.tolist() for v in grid_team_clearance([a, b], 2)] == [[1], [1]]
    assert [v.tolist() for v in grid_team_clearance([a, [(1, 0), (1, 0)]], 2)] == [[1], [0]]
    assert [v.tolist() for v in grid_team_clearance([a, [(1, 1), (0, 0)]], 2)] == [[0], [0]]          # a swap along one diagonal: no crossing, clearance 0
    assert [v.tolist() for v in grid_team_clearance([a, [(5, 5), (6, 6)]], 2)] == [[4], [0]]   # (1, 1) to (5, 5)
    # the tail: with T = 1 the cells from c[1] on of both walks are compared pair by pair, whatever their action
    w0, w1 = [(0, 0), (1, 0), (2, 0), (3, 0)], [(9, 0), (9, 1), (9, 2), (3, 3)]
    assert grid_team_clearance([w0, w1], 2)[0].tolist() == [3] and grid_team_clearance([w0, w1], 2, 1)[0].tolist() == [3]
    assert grid_team_clearance([w0, [(9, 5), (9, 4), (3, 2), (9, 9)]], 2)[0].tolist() == [2]
    assert grid_team_clearance([w0, [(9, 5), (9, 4), (3, 2), (9, 9)]], 2, 1)[0].tolist() == [2]
    assert grid_team_clearance([w0, [(9, 5), (9, 4), (9, 9), (0, 1)]], 2)[0].tolist() == [2]
    assert grid_team_clearance([w0, [(9, 5), (9, 4), (9, 9), (0, 1)]], 2, 1)[0].tolist() == [1]   # (1, 0) of the tail meets (0, 1), whenever
    assert grid_team_clearance([w0], 1)[0].tolist() == [R.PLAN_NO_PAIR]
    assert grid_team_clearance([w0, w1, w0, w0], 2)[0].tolist() == [3, 0]
    with pytest.raises(ValueError, match="do not split"):
        grid_team_clearance([w0, w1, w0], 2)


def test_size_one_equals_the_time_plan_and_one_frame_equals_the_static_plan():
    spec, walls, hz, scene, start, goal = circling33()
    ref = grid_plan_time(spec, walls, hz, start, goal, 4, 0, 10, 8)
    out = grid_plan_team(spec, walls, hz, start, goal, 4, teams(1), 2, 0, 10, 8)
    same_time(out, ref, ("occupancy", "layer_first", "layer_number"))
    gx, gy = spec.cell_of(goal)
    col = ref["occupancy"][scene, :, gy, gx]                                      # [n][T + 1]: the goal cell through the layers
    keeps = np.array([not any(not col[i, t] and col[i, t + 1:].any() for t in range(8)) for i in range(33)])   # no layer blocks a goal cell an earlier one left free
    assert keeps.sum() >= 25
    for k in TIME:
        assert np.array_equal(out[k][keeps].view(np.uint32), ref[k][keeps].view(np.uint32)), k
    assert np.array_equal(out["fields"][keeps], ref["fields"][ref["field_of"]][keeps]) and np.all(out["team_clearance"] == R.PLAN_NO_PAIR)
    h3 = three_hazards(scene)
    one = MovingHazards(h3.table[:, None, :, :2].astype(np.float64), size=h3.table[:, :, 2].astype(np.float64), counts=h3.counts, scene=scene)
    static = grid_plan(spec, walls, h3, start, goal, 4)
    for hazards in (one, h3):                                                    # a one-frame table, and the static hazards themselves
        out = grid_plan_team(spec, walls, hazards, start, goal, 4, teams(1), 0, 5, 3, 5)
        same_time(out, static, PLAN)
        for t in range(6):
            assert np.array_equal(out["fields"][:, t], static["fields"][static["field_of"]]) and np.array_equal(out["occupancy"][:, t], static["occupancy"])
    out = grid_plan_team(spec, walls, None, start, goal, 4, teams(1), 0, 0, 3, 2)  # no hazards at all
    same_time(out, grid_plan(spec, walls, None, start, goal, 4), PLAN)


@pytest.mark.parametrize("r", [0, 1])
def test_a_goal_an_earlier_mate_crosses_later_is_not_terminal_before_the_crossing(r):
    spec, start, goal = crossing_goal_case()
    out = grid_plan_team(spec, None, None, start, goal, 8, teams(2), r, 0, 10, 48)
    w0, w1 = (np.array(w) for w in out["walks"])
    assert out["status"].tolist() == [0, 0] and out["arrive"][0] == 24 and np.array_equal(w0[12], (16, 16))
    alone = alone_walks(spec, start, goal, 48)[1]
    assert len(alone) - 1 == 3                                                   # it could arrive at action 3 ...
    assert out["arrive"][1] > 12 + r and (out["waits"][1].sum() > 0 or len({tuple(c) for c in w1}) > 4)   # ... and waits or steps off instead
    first_on_goal = min(a for a in range(len(w1)) if tuple(w1[a]) == (16, 16))
    assert first_on_goal > 12, "the walk must not end on the goal before the mate has passed"
    clear, cross = grid_team_clearance(out["walks"], 2, 48)
    assert clear[0] > r and cross[0] == 0
    g = 16 * 32 + 16
    f1 = out["fields"][1].reshape(49, -1)
    assert np.all(f1[13 + r:, g] == 0) and not np.any(f1[:12 - r, g] == 0)       # terminal only once it stays free
    # grid_time_field's rule would have made it terminal at once: that is the one change
    layers = out["occupancy"][0] | R.grid_reserve(out["walks"][0], 48, 32, r)
    assert R.grid_time_field(layers, g)[0, 16, 16] == 0 and R.grid_team_field(layers, g)[0, 16, 16] > 0


def test_a_parked_mate_reserves_its_start_cell_in_every_layer():
    spec, walls, start, goal = sealed_case()
    out = grid_plan_team(spec, walls, None, start, goal, 8, teams(2), 1, 0, 10, 24)
    assert out["status"].tolist() == [R.UNREACHABLE, R.PLANNED] and out["walks"][0] == [(9, 24)] and out["arrive"].tolist() == [0, 8]
    assert out["count"][0] == 0 and out["cost"][0] == -1 and not out["waypoints"][0].any()
    assert np.all(out["fields"][1][:, 23:26, 8:11] == -1)                        # reserved in every layer, the tail too
    straight = grid_plan_team(spec, walls, None, start[1:], goal[1:], 8, teams(1), 1, 0, 10, 24)
    assert straight["arrive"][0] == 8 and straight["cost"][0] == 40 and out["cost"][1] > 40    # member 1 routes round it
    assert out["team_clearance"][0] == 2 and out["team_crossings"][0] == 0


def test_stated_incompleteness_a_later_member_within_reserve_of_an_earlier_start_is_unreachable():
    start = centres(SPEC32, [(8, 16), (9, 17)])
    goal = centres(SPEC32, [(20, 16), (9, 26)])
    assert grid_plan_team(SPEC32, None, None, start, goal, 8, teams(2), 0, 0, 10, 24)["status"].tolist() == [0, 0]
    out = grid_plan_team(SPEC32, None, None, start, goal, 8, teams(2), 1, 0, 10, 24)
    assert out["status"].tolist() == [R.PLANNED, R.UNREACHABLE] and out["walks"][1] == [(9, 17)]
    # and the other way round nothing is promised either: the earlier member does not know the later one's start
    assert out["team_clearance"][0] == 1


def test_truncated_members_reserve_their_walk_and_release_steps_follow_the_waits():
    spec, walls, hz, start, goal = circling32()
    out = grid_plan_team(spec, walls, hz, start, goal, 4, teams(4), 1, 7, 10, 8)
    assert {R.PLANNED, R.UNREACHABLE, R.TRUNCATED} <= set(out["status"].tolist()) and out["waits"].sum() > 0
    assert np.array_equal(out["release"], R.grid_release(out["waits"], out["leave"], 7, 10))
    i = int(np.flatnonzero(out["status"] == R.TRUNCATED)[0])
    assert len(out["walks"][i]) == out["arrive"][i] + 1 > 1 and out["count"][i] > 4
    planned = np.isin(out["status"], (R.PLANNED, R.TRUNCATED))
    for g in range(8):                                                           # between members that have a walk the guarantee holds
        members = [j for j in range(4 * g, 4 * g + 4) if planned[j]]
        if len(members) > 1:
            clear, cross = grid_team_clearance([out["walks"][j] for j in members], len(members), 8)
            assert clear[0] > 1 and cross[0] == 0


def test_rule_refusals_are_named():
    spec, walls, hz, start, goal = circling32()
    kw = dict(step0=0, layer_steps=10, layers=8)
    for r in (-1, 5, 1.0, True):
        with pytest.raises(ValueError, match="reserve"):
            grid_plan_team(spec, walls, hz, start, goal, 4, teams(2), r, **kw)
    with pytest.raises(ValueError, match="team size"):
        Teams(3, 0.1)
    with pytest.raises(ValueError, match="do not split"):
        grid_plan_team(spec, None, None, start[:6], goal[:6], 4, teams(4), 1, **kw)
    with pytest.raises(TypeError, match="Teams"):
        grid_plan_team(spec, walls, hz, start, goal, 4, 2, 1, **kw)
    with pytest.raises(ValueError, match="layer_steps and layers are required"):
        grid_plan_team(spec, walls, None, start, goal, 4, teams(2), 1)
    for change, word in ((dict(layers=0), "layers"), (dict(layers=257), "layers"), (dict(layer_steps=0), "layer_steps"), (dict(step0=-1), "step0")):
        with pytest.raises(ValueError, match=word):
            grid_plan_team(spec, walls, hz, start, goal, 4, teams(2), 1, **dict(kw, **change))
    with pytest.raises(ValueError, match="one scene"):                            # scenes that alternate robot by robot
        grid_plan_team(spec, two_scenes(np.arange(32) % 2), None, start, goal, 4, teams(2), 1, **kw)
    with pytest.raises(ValueError, match="agree on the scene"):
        grid_plan_team(spec, two_scenes(1 - np.arange(32) // 16), hz, start, goal, 4, teams(2), 1, **kw)
    with pytest.raises(ValueError, match="exceed the cap"):                       # 64 fields of 257 x 128 x 128 x 4 bytes asked for
        grid_plan_team(GridSpec(EXTENT, 128), None, None, np.zeros((64, 2), np.float32), np.zeros((64, 2), np.float32), 4, teams(2), 1, 0, 1, 256)


def test_planner_host_path_defaults_and_refusals():
    spec, start, goal = swap_case()
    with pytest.raises(ValueError, match="layer_steps"):
        GridPlanner("point", teams=teams(2), cells=32, extent=EXTENT)
    with pytest.raises(ValueError, match="smooth"):
        GridPlanner("point", teams=teams(2), cells=32, extent=EXTENT, layer_steps=10, smooth=True)
    with pytest.raises(ValueError, match="reserve= belongs to teams"):
        GridPlanner("point", cells=32, extent=EXTENT, reserve=1)
    with pytest.raises(TypeError, match="Teams"):
        GridPlanner("point", teams=2, cells=32, extent=EXTENT, layer_steps=10)
    with pytest.raises(ValueError, match="reserve"):
        GridPlanner("point", teams=teams(2), reserve=5, cells=32, extent=EXTENT, layer_steps=10)
    h = float(SPEC32.h)                                                           # 0.125: ceil(separation / h)
    for sep, r in ((0.0, 0), (0.1, 1), (0.125, 1), (0.13, 2), (0.3, 3), (0.5, 4)):
        assert GridPlanner("point", teams=Teams(2, sep), cells=32, extent=EXTENT, layer_steps=10).reserve == r == int(np.ceil(np.float32(sep) / h))
    with pytest.raises(ValueError, match="coarser grid"):
        GridPlanner("point", teams=Teams(2, 0.51), cells=32, extent=EXTENT, layer_steps=10)
    planner = GridPlanner("point", teams=teams(2), cells=32, inflate=INFLATE, extent=EXTENT, layer_steps=10, layers=48, max_waypoints=8)
    assert not planner.device and planner.reserve == 1 and planner.timed
    got = planner.plan(start, goal, want_fields=True, want_occupancy=True)
    ref = grid_plan_team(spec, None, None, start, goal, 8, teams(2), 1, 0, 10, 48)
    same_team(got, ref)
    assert got["team_clearance"].tolist() == [2] and np.array_equal(got["schedule"].release, ref["release"])
    with pytest.raises(ValueError, match="smooth"):
        planner.plan(start, goal, smooth=True)
    with pytest.raises(ValueError, match="horizon"):
        planner.callback(goal)


def test_team_callback_replans_the_whole_team_of_a_stalled_member_without_its_finished_members():
    from mobrob_amd.waypoints import FINISHED, GOING, STALLED
    spec, start, goal = lattice_case()
    planner = GridPlanner("point", teams=teams(4), reserve=1, cells=32, inflate=INFLATE, extent=EXTENT, layer_steps=10, layers=48, max_waypoints=16)
    cb = planner.callback(goal, horizon=30)
    status = np.full(16, GOING)
    assert cb(start, status, np.zeros(16, np.int32)) == {} and cb.calls == 1
    status[5], status[6], status[9] = STALLED, FINISHED, FINISHED
    where = start.copy()
    where[6], where[9] = goal[6], goal[9]
    rows = cb(where, status, np.zeros(16, np.int32))
    assert sorted(rows) == [4, 5, 7] and cb.calls == 2                            # team 1 without its finished member; team 2 has no stalled one
    ref = grid_plan_team(spec, None, None, where, goal, 16, teams(4), 1, 60, 10, 48)
    for i, (w, rel) in rows.items():
        m = ref["n_waypoints"][i]
        assert w.view(np.uint32).tobytes() == ref["waypoints"][i, :m].view(np.uint32).tobytes() and np.array_equal(rel, ref["release"][i, :m])
    assert ref["arrive"][6] == 0 and cb.last["team_clearance"][1] > 1             # the finished member is planned where it stands
