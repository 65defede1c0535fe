"""CPU: the rule of line-of-sight smoothing over time (goal_rules.grid_next_blocked, grid_los_time, grid_smooth_time,
grid_path_smooth_time, grid_release_smooth, grid_plan_time(smooth=True)): a straight leg is tested against every layer it spans.
All integers, so nothing here has a tolerance; the guarantee is checked by brute force, layer by layer, with grid_los's own walk."""
import numpy as np
import pytest

from mobrob_amd.envs import goal_rules as R
from mobrob_amd.envs.goal_rules import grid_plan, grid_plan_time
from mobrob_amd.planning import GridPlanner
from mobrob_amd.waypoints import follow_with_replanning
from tests.plan_scenes import EXTENT, INFLATE
from tests.plan_smooth_cases import same_plan
from tests.plan_time_scenes import circling33, gap_case, goal_sitter, same_time
from tests.plan_time_smooth_cases import SMOOTH_KEYS, cap_boundary, kept_and_cells, scenes, static_twin


def test_next_blocked_is_the_first_blocked_layer_from_t_on():
    rng = np.random.default_rng(11)
    blk = rng.random((4, 8, 8)) < 0.3
    nb = R.grid_next_blocked(blk)
    assert nb.dtype == np.int16 and nb.shape == blk.shape
    for lo in range(4):
        for hi in range(lo, 4):
            assert np.array_equal(nb[lo] > hi, ~blk[lo:hi + 1].any(axis=0)), (lo, hi)
    assert set(np.unique(nb)) <= {0, 1, 2, 3, R.PLAN_NEVER_BLOCKED} and np.all(nb[3][~blk[3]] == 32767)


def test_los_time_is_symmetric_and_is_grid_los_on_the_or_of_the_layers():
    rng = np.random.default_rng(12)
    blk = rng.random((4, 8, 8)) < 0.12
    nb = R.grid_next_blocked(blk)
    seen = set()
    for _ in range(300):
        a, b = tuple(rng.integers(0, 8, 2)), tuple(rng.integers(0, 8, 2))
        lo = int(rng.integers(0, 4))
        hi = int(rng.integers(lo, 4))
        got = R.grid_los_time(nb, a, b, lo, hi)
        assert got == R.grid_los_time(nb, b, a, lo, hi) == R.grid_los(blk[lo:hi + 1].any(axis=0), a, b, 0)
        seen.add(got)
    assert seen == {True, False}


@pytest.mark.parametrize("margin", [0, 1])
@pytest.mark.parametrize("name", ["circling33_3_64", "circling33_10_32", "gap_case", "goal_sitter"])
def test_every_kept_leg_of_two_or_more_actions_is_visible_in_each_layer_of_its_span(name, margin):
    spec, walls, hz, start, goal, ls, T = scenes()[name]
    plan = grid_plan_time(spec, walls, hz, start, goal, 64, 0, ls, T, smooth=True, margin=margin, want_next_blocked=True)
    assert not np.any(plan["status"] == R.TRUNCATED) and np.any(plan["status"] == R.PLANNED) and not plan["waits"].any()
    legs = spans = 0
    for i in range(len(start)):
        cells, acts, keep = kept_and_cells(plan, spec, start, goal, i)
        if not cells:
            assert plan["status"][i] == R.UNREACHABLE and plan["count"][i] == 0 and plan["cost"][i] == -1 and not plan["waypoints"][i].any()
            continue
        s = plan["field_scene"][plan["field_of"][i]]
        A = len(cells) - 1
        assert plan["arrive"][i] == A and plan["moves"][i] == sum(k != R.PLAN_WAIT_ACTION for k in acts) and plan["count"][i] == len(keep) + 1
        assert plan["leave"][i, :len(keep) + 1].tolist() == [0] + keep and not plan["leave"][i, len(keep) + 1:].any()
        ends = [0] + keep + [A]
        for a, b in zip(ends[:-1], ends[1:]):
            assert b > a or A == 0                              # (a start in the goal's cell: no action, the goal alone)
            if b - a < 2:
                continue
            legs += 1
            for t in range(min(a, T), min(b, T) + 1):          # brute force: the static rule's own walk, a layer at a time
                spans += 1
                blk = R.los_blocked(plan["occupancy"][s, t], margin)
                assert R.los_walk(blk, cells[a], cells[b])[0], (i, a, b, t)
    print(name, "margin", margin, "count", int(plan["count"].sum()), "legs of >= 2 actions", legs, "layer tests", spans)
    if (name, margin) == ("gap_case", 1):                      # a walk along blocked cells keeps every cell: no leg to test
        assert legs == 0 and plan["count"][0] == plan["arrive"][0] == 9
    else:
        assert legs > 0 and spans > legs


@pytest.mark.parametrize("margin", [0, 1])
def test_one_frame_is_the_static_smoother_bit_for_bit(margin):
    spec, walls, one, h_static, start, goal = static_twin()
    ref = grid_plan(spec, walls, h_static, start, goal, 64, smooth=True, margin=margin)
    got = grid_plan_time(spec, walls, one, start, goal, 64, step0=3, layer_steps=5, layers=6, smooth=True, margin=margin)
    same_plan(got, ref)
    assert np.sum(ref["moves"] > 2) >= 10 and np.array_equal(got["arrive"], got["moves"])


def test_spans_past_the_tail_collapse_onto_layer_t():
    spec, walls, hz, scene, start, goal = circling33()
    plan = grid_plan_time(spec, walls, hz, start, goal, 64, 0, 3, 4, smooth=True, margin=0, want_next_blocked=True)
    long = np.flatnonzero(plan["arrive"] > 20)
    assert long.size > 0
    for i in long:
        cells, _, keep = kept_and_cells(plan, spec, start, goal, i)
        s = plan["field_scene"][plan["field_of"][i]]
        tail = R.los_blocked(plan["occupancy"][s, 4], 0)
        past = [0] + [j for j in keep if j >= 4]
        assert len(past) > 1
        # beyond T the rule is the static smoother on the tail's map, from the first anchor at or past T on
        first = next(j for j in keep if j >= 4)
        assert [first + j for j in R.grid_smooth(cells[first:], None, blocked=tail)] == [j for j in keep if j > first]
        assert np.all(plan["next_blocked"][s, 4][tail] == 4) and np.all(plan["next_blocked"][s, 4][~tail] == 32767)


def test_release_holds_at_every_anchor_but_the_start():
    leave = np.array([[0, 3, 7, 0], [0, 0, 0, 0]], np.int32)
    rel = R.grid_release_smooth(leave, 5, 10)
    assert rel.dtype == np.int32 and rel.tolist() == [[0, 35, 75, 0], [0, 0, 0, 0]]
    with pytest.raises(ValueError, match="fit an int32"):
        R.grid_release_smooth(np.array([[0, 16000]]), 0, 2 ** 20)
    spec, hz, start, goal = goal_sitter()
    plan = grid_plan_time(spec, None, hz, start, goal, 4, 20, 10, 16, smooth=True, margin=0)
    raw = grid_plan_time(spec, None, hz, start, goal, 4, 20, 10, 16)
    assert plan["count"][0] == 2 and plan["leave"][0].tolist() == [0, 8, 0, 0] and plan["release"][0].tolist() == [0, 100, 0, 0]
    assert np.all(plan["release"][:, 0] == 0) and raw["count"][0] == 1 and plan["arrive"][0] == raw["arrive"][0] == 10
    for k in ("occupancy", "fields", "cost", "arrive", "layer_first", "layer_number"):
        assert np.array_equal(plan[k], raw[k]), k
    with pytest.raises(ValueError, match="margin must be 0 or 1"):
        grid_plan_time(spec, None, hz, start, goal, 4, 0, 10, 16, smooth=True, margin=2)
    # the cap at its boundary: 15 fields over 2 scenes at G = 128, T = 256 fit alone (240.9 MiB) and not with the table (257.0 MiB)
    bspec, bhz, bstart, bgoal, bls, bT = cap_boundary()
    assert len(R.plan_fields(bspec, None, bhz.scene, bgoal)[1]) == 15 and R.plan_scene_time(None, bhz)[0] == 2
    with pytest.raises(ValueError, match="next-blocked table of 2 x 257 x 128 x 128 x 2"):
        grid_plan_time(bspec, None, bhz, bstart, bgoal, 2, 0, bls, bT, smooth=True)
    assert 15 * (bT + 1) * 128 * 128 * 4 <= R.PLAN_TIME_MAX_BYTES                 # the unsmoothed plan's own check accepts the shape ...
    R.plan_time_smooth_check(15, 1, bT, 128, 1)                                  # ... and so does the smoothed one with one scene's table
    with pytest.raises(ValueError, match="next-blocked table"):
        R.plan_time_smooth_check(15, 2, bT, 128, 1)


def test_planner_on_an_env_name():
    spec, walls, hz, scene, start, goal = circling33()
    kw = dict(walls=walls, hazards=hz, cells=32, inflate=INFLATE, extent=EXTENT, layer_steps=10, layers=32)
    for margin in (0, 1):
        planner = GridPlanner("point", max_waypoints=64, time_smooth=True, los_margin=margin, **kw)
        got = planner.plan(start, goal, want_occupancy=True, want_fields=True)
        ref = grid_plan_time(spec, walls, hz, start, goal, 64, 0, 10, 32, smooth=True, margin=margin)
        same_time(got, ref, SMOOTH_KEYS + ("occupancy", "fields"))
        assert got["smoothed"] and isinstance(got["schedule"], R.Schedule) and np.array_equal(got["schedule"].release, ref["release"])
        assert np.array_equal(got["schedule"].home, start) and not got["waits"].any() and not got["fields_reused"]
    plain = GridPlanner("point", max_waypoints=64, **kw)
    today = grid_plan_time(spec, walls, hz, start, goal, 64, 0, 10, 32)
    for got in (plain.plan(start, goal), planner.plan(start, goal, time_smooth=False), plain.plan(start, goal, time_smooth=False)):
        same_time(got, today, ("waypoints", "n_waypoints", "count", "status", "cost", "waits", "leave", "arrive", "release"))
        assert not got["smoothed"] and got["moves"] is None
    same_time(plain.plan(start, goal, time_smooth=True), ref, SMOOTH_KEYS)                      # per call, at the planner's margin (1)
    # grow: K = 2 truncates; the second plan has the smoothed count's slots
    two = GridPlanner("point", max_waypoints=2, time_smooth=True, los_margin=0, **kw)
    ref2 = grid_plan_time(spec, walls, hz, start, goal, 2, 0, 10, 32, smooth=True, margin=0)
    same_time(two.plan(start, goal), ref2, SMOOTH_KEYS)
    assert np.any(ref2["status"] == R.TRUNCATED) and np.all(ref2["leave"][:, 0] == 0)
    grown = two.plan(start, goal, grow=True)
    same_time(grown, grid_plan_time(spec, walls, hz, start, goal, int(ref2["count"].max()), 0, 10, 32, smooth=True, margin=0), SMOOTH_KEYS)
    assert grown["waypoints"].shape[1] == ref2["count"].max() > 2 and not np.any(grown["status"] == R.TRUNCATED)


def test_planner_refusals_are_named():
    spec, walls, hz, start, goal = gap_case()
    kw = dict(walls=walls, cells=32, extent=EXTENT)
    with pytest.raises(ValueError, match="time_smooth"):
        GridPlanner("point", hazards=hz, layer_steps=10, smooth=True, **kw)                       # smooth= still raises, and names the keyword
    with pytest.raises(ValueError, match="time_smooth=True needs"):
        GridPlanner("point", time_smooth=True, **kw)                                              # no moving hazards
    with pytest.raises(ValueError, match="time_smooth=True needs"):
        GridPlanner("point", hazards=R.Hazards(np.array([[[0.5, 0.5]]]), size=0.1), time_smooth=True, **kw)
    with pytest.raises(ValueError, match="time_smooth=True needs"):
        GridPlanner("point", hazards=hz, teams=R.Teams(1, 0.1), layer_steps=10, time_smooth=True, **kw)
    timed = GridPlanner("point", hazards=hz, layer_steps=10, **kw)
    with pytest.raises(ValueError, match="smooth"):
        timed.plan(start, goal, smooth=True)
    with pytest.raises(ValueError, match="time_smooth=True needs"):
        GridPlanner("point", **kw).plan(start, goal, time_smooth=True)
    with pytest.raises(ValueError, match="time_smooth=True needs"):
        GridPlanner("point", hazards=hz, teams=R.Teams(1, 0.1), layer_steps=10, **kw).plan(start, goal, time_smooth=True)
    assert GridPlanner("point", hazards=hz, layer_steps=10, time_smooth=True, **kw).time_smooth and not timed.time_smooth


def test_replanning_rounds_through_the_callback():
    from tests.test_teams_cpu import _GoToGoal
    spec, walls, hz, start, goal = gap_case(stay=30)
    rng = np.random.default_rng(3)
    start = rng.uniform(-1.4, 1.4, (6, 2)).astype(np.float32)
    start[:, 0] = -np.abs(start[:, 0]) - 0.15                                    # left of the thin wall, goals right of it
    goal = np.tile(np.array([[1.2, 1.2], [1.3, -0.2]], np.float32), (3, 1))
    planner = GridPlanner("point", walls=walls, hazards=hz, cells=32, inflate=INFLATE, max_waypoints=16, extent=EXTENT, layer_steps=5, layers=16,
                          time_smooth=True, los_margin=0)
    first = planner.plan(start, goal)
    assert np.sum(first["status"] == R.PLANNED) >= 4 and first["smoothed"] and np.any(first["release"] > 0)
    inner, calls = planner.callback(goal, horizon=20), []

    def recording(positions, status, reached):
        new = inner(positions, status, reached)
        calls.append(new)
        return new
    out = follow_with_replanning(_GoToGoal(), "point", start, first["waypoints"], recording, horizon=20, rounds=3, leg_steps=7,
                                 n_waypoints=first["n_waypoints"], seed=1, hazards=hz, walls=walls, schedule=first["schedule"])
    assert len(calls) == 2 and inner.calls == 2 and out["state"].step0 == 60
    assert sum(len(c) for c in calls) > 0, "a leg budget of 7 steps stalls robots: the loop must have replanned some"
    for r, new in enumerate(calls):
        for i, (w, rel) in new.items():
            assert len(w) == len(rel) and rel[0] == 0 and np.all(rel[1:] > 20 * (r + 1))          # holds at every anchor but the start
    assert inner.last["smoothed"] and not inner.last["waits"].any()
