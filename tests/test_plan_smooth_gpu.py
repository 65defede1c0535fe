"""GPU: line-of-sight smoothing on the device (mobrob_ppo_plan_smooth: k_plan_dilate, k_plan_smooth) against the NumPy rule
(goal_rules.grid_plan(smooth=True)), BIT FOR BIT: float32 waypoints compared as uint32; n_waypoints, counts, statuses, costs and
moves as integers.  Nothing here has a tolerance: the rule is integer arithmetic on the occupancy the device keeps resident."""
import numpy as np
import pytest

from mobrob_amd.envs import goal_rules as R
from mobrob_amd.envs.goal_rules import GridSpec, Hazards, Walls, grid_plan
from mobrob_amd.planning import GridPlanner
from mobrob_amd.waypoints import STALLED, follow_with_replanning
from tests.plan_scenes import EXTENT, INFLATE, SCENE0, robots8_xyz, robots33, serpentine, three_hazards, two_scenes, xyz_checked
from tests.plan_smooth_cases import KEYS, corners_met, same_plan, window_edges
from tests.util import _engine, _env, _snapshot, golden_params, load_golden

pytestmark = pytest.mark.gpu
KW = dict(pi=(64, 64), vf=(64, 64))


@pytest.fixture(scope="module")
def engine():
    e, _ = _engine("point", KW)
    yield e
    e.close()


def smooth_both(engine, spec, walls, hazards, start, goal, K, margin):
    """-> (device, rule): plan_grid, then plan_smooth on its resident fields; the rule on the device's own occupancy and fields
    (compared with the rule's own by tests/test_plan_gpu.py)"""
    full = engine.plan_grid(spec, walls, hazards, start=start, goal=goal, max_waypoints=K, want_occupancy=True, want_fields=True)
    dev = engine.plan_smooth(spec, reuse=full, start=start, goal=goal, scene=R.plan_scene(walls, hazards)[1], max_waypoints=K, margin=margin)
    ref = grid_plan(spec, walls, hazards, start, goal, K, full["occupancy"], full["fields"], smooth=True, margin=margin)
    return dev, ref, full


@pytest.mark.parametrize("margin", [0, 1])
@pytest.mark.parametrize("scene_kind", ["walls", "walls_hazards", "hazards", "empty"])
def test_g32_two_scenes_33_robots(engine, scene_kind, margin):
    scene, start, goal = robots33()
    walls = two_scenes(scene) if scene_kind.startswith("walls") else None
    hazards = three_hazards(scene) if "hazards" in scene_kind else None
    spec = GridSpec(EXTENT, 32, INFLATE if walls is not None else None)
    dev, ref, full = smooth_both(engine, spec, walls, hazards, start, goal, 4, margin)
    same_plan(dev, ref)
    assert np.any(ref["moves"] > 2) and np.any(ref["status"] == R.PLANNED)
    if scene_kind == "walls":                                       # (at margin 0 no smoothed plan here needs more than K = 4)
        assert set(ref["status"].tolist()) == ({R.PLANNED, R.UNREACHABLE, R.TRUNCATED} if margin == 1 else {R.PLANNED, R.UNREACHABLE})
    if scene_kind == "empty":
        assert np.all(dev["count"] == 1)
    if margin == 0:
        assert np.all(dev["count"] <= full["count"])


def test_g32_three_column_starts_and_goals(engine):
    spec, walls, _, start, goal = robots8_xyz()
    dev, ref, _ = smooth_both(engine, spec, walls, None, start, goal, 2, 0)
    same_plan(dev, xyz_checked(ref, goal, 2))


def test_g128_walks_longer_than_one_window(engine):
    rng = np.random.default_rng(5)
    walls = Walls(SCENE0, radius=0.05)
    goals = np.array([(1.2, 1.2), (-1.2, -1.2), (1.2, -1.3), (-0.3, 1.3)], np.float32)
    start = rng.uniform(-1.5, 1.5, (9, 2)).astype(np.float32)
    goal = goals[np.arange(9) % 4]
    spec = GridSpec(EXTENT, 128)
    for margin in (0, 1):
        dev, ref, _ = smooth_both(engine, spec, walls, None, start, goal, 12, margin)
        same_plan(dev, ref)
        assert np.sum(ref["moves"] > 64) >= 2, "the window of 64 candidates must refill"


@pytest.mark.parametrize("margin", [0, 1])
def test_g64_serpentine_slides_the_window_with_a_moving_anchor(engine, margin):
    spec, walls, start, goal = serpentine()
    dev, ref, full = smooth_both(engine, spec, walls, None, start, goal, 64, margin)
    print("serpentine margin", margin, "moves", dev["moves"], "count", dev["count"], "unsmoothed", full["count"])
    same_plan(dev, ref)
    assert ref["moves"][0] == 656 and ref["count"][0] > 10


def test_window_edges_63_64_65_127_128_129_moves(engine):
    spec, walls, start, goal, want = window_edges()
    for margin in (0, 1):
        dev, ref, _ = smooth_both(engine, spec, walls, None, start, goal, 16, margin)
        assert np.array_equal(ref["moves"], want)
        same_plan(dev, ref)


def test_the_corner_branch_of_the_rule_fires(engine):
    scene, start, goal = robots33()
    for walls, spec in ((None, GridSpec(EXTENT, 32)), (two_scenes(scene), GridSpec(EXTENT, 32, INFLATE))):
        dev, ref, full = smooth_both(engine, spec, walls, None, start, goal, 8, 0)
        n = corners_met(full, spec, start, goal, 0)
        print("t == 0 met", n, "times")
        assert n > 0
        same_plan(dev, ref)


def test_truncation_grow_rounds_and_the_unsmoothed_bits_on_the_planner(engine):
    scene, start, goal = robots33()
    walls = two_scenes(scene)
    env = _env("point", 33)
    planner = GridPlanner(env, walls=walls, cells=32, inflate=INFLATE, max_waypoints=2, engine=engine, extent=EXTENT, smooth=True, los_margin=0)
    spec = planner.spec
    raw2 = grid_plan(spec, walls, None, start, goal, 2)
    sm2 = grid_plan(spec, walls, None, start, goal, 2, smooth=True, margin=0)
    gain = (raw2["status"] == R.TRUNCATED) & (sm2["status"] == R.PLANNED)
    assert gain.any() and np.any(sm2["status"] == R.TRUNCATED)
    got = planner.plan(start, goal)
    same_plan(got, sm2)
    assert got["smoothed"] and not got["fields_reused"] and np.all(got["status"][gain] == R.PLANNED)
    grown = planner.plan(start, goal, grow=True)
    same_plan(grown, grid_plan(spec, walls, None, start, goal, int(sm2["count"].max()), smooth=True, margin=0))
    assert grown["waypoints"].shape[1] == sm2["count"].max() < raw2["count"].max() and not np.any(grown["status"] == R.TRUNCATED)
    # a replanning round: new starts, the same goals -> k_plan_smooth alone on the resident fields
    moved = start[::-1].copy()
    again = planner.plan(moved, goal)
    assert again["fields_reused"] and again["smoothed"]
    same_plan(again, grid_plan(spec, walls, None, moved, goal, 2, smooth=True, margin=0))
    # an unsmoothed plan after a smoothed one: the old bits, by k_plan_path on the same fields
    plain = planner.plan(start, goal, smooth=False)
    same_plan(plain, raw2, KEYS[:-1])
    assert plain["fields_reused"] and not plain["smoothed"] and plain["moves"] is None
    fresh = GridPlanner(env, walls=walls, cells=32, inflate=INFLATE, max_waypoints=2, engine=engine, extent=EXTENT)
    same_plan(fresh.plan(start, goal), raw2, KEYS[:-1])
    # margin 1 on the same planner settings: the dilated map is made once and kept
    m1 = GridPlanner(env, walls=walls, cells=32, inflate=INFLATE, max_waypoints=2, engine=engine, extent=EXTENT, smooth=True)
    same_plan(m1.plan(start, goal), grid_plan(spec, walls, None, start, goal, 2, smooth=True, margin=1))
    same_plan(m1.plan(moved, goal), grid_plan(spec, walls, None, moved, goal, 2, smooth=True, margin=1))


def test_refusals_are_named_before_any_launch(engine):
    scene, start, goal = robots33()
    walls = two_scenes(scene)
    spec = GridSpec(EXTENT, 32, INFLATE)
    ok = engine.plan_grid(spec, walls, None, start=start, goal=goal, max_waypoints=4)
    kw = dict(start=start, goal=goal, scene=scene, max_waypoints=4)
    good = engine.plan_smooth(spec, reuse=ok, margin=0, **kw)
    with pytest.raises(ValueError, match="margin must be 0 or 1"):
        engine.plan_smooth(spec, reuse=ok, margin=2, **kw)
    with pytest.raises(ValueError, match="max_waypoints"):
        engine.plan_smooth(spec, reuse=ok, margin=0, start=start, goal=goal, scene=scene, max_waypoints=0)
    with pytest.raises(ValueError, match="resident fields"):
        engine.plan_smooth(spec, reuse=ok, margin=0, start=start, goal=goal, scene=np.full(33, 5), max_waypoints=4)
    with pytest.raises(Exception, match="no longer resident"):
        engine.plan_smooth(spec, reuse=dict(ok, fields_id=0), margin=0, **kw)
    same_plan(engine.plan_smooth(spec, reuse=ok, margin=0, **kw), good)          # a refused call changes nothing
    engine.plan_grid(GridSpec(EXTENT, 64, INFLATE), walls, None, start=start, goal=goal, max_waypoints=4)   # replaces the resident fields
    with pytest.raises(Exception, match="no longer resident"):
        engine.plan_smooth(spec, reuse=ok, margin=0, **kw)


def test_training_untouched_by_smooth_calls():
    scene, start, goal = robots33()
    walls = two_scenes(scene)
    spec = GridSpec(EXTENT, 32, INFLATE)
    env_a, env_b = _env("point", 16, tl=40), _env("point", 16, tl=40)
    ea, _ = _engine("point", KW, seed=7)
    eb, _ = _engine("point", KW, seed=7)
    out = None
    for it in range(2):
        env_a.collect(ea)
        env_b.collect(eb)
        before = _snapshot(eb, stats=False)
        kept = eb.plan_grid(spec, walls, three_hazards(scene), start=start, goal=goal, max_waypoints=4)
        for margin in (0, 1):
            out = eb.plan_smooth(spec, reuse=kept, start=start[::-1].copy(), goal=goal, scene=scene, max_waypoints=4, margin=margin)
        sa, sb = _snapshot(ea, stats=False), _snapshot(eb, stats=False)
        for k in sa:
            assert np.array_equal(sa[k], sb[k]) and np.array_equal(before[k], sb[k]), f"iteration {it}: {k} differs"
        ea.train()
        eb.train()
        assert np.array_equal(ea.get_flat_params(), eb.get_flat_params())
    assert np.any(out["status"] == R.PLANNED)
    ea.close()
    eb.close()


def test_replanning_loop_with_smoothing_equals_the_loop_driven_by_the_rule():
    e, _ = _engine("point", KW)
    e.set_params(golden_params(load_golden("point")))
    rng = np.random.default_rng(3)
    walls = Walls(SCENE0, radius=0.05)
    start = rng.uniform(-1.4, 1.4, (32, 2)).astype(np.float32)
    start[:, 0] = -np.abs(start[:, 0]) - 0.15
    goal = np.tile(np.array([[1.2, 1.2], [1.3, -0.2]], np.float32), (16, 1))
    planner = GridPlanner(_env("point", 32), walls=walls, cells=32, inflate=INFLATE, max_waypoints=8, engine=e, extent=EXTENT, smooth=True,
                          los_margin=0)
    spec = planner.spec
    first = planner.plan(start, goal)
    ref_first = grid_plan(spec, walls, None, start, goal, 8, smooth=True, margin=0)
    same_plan(first, ref_first)
    replanned = []

    def by_the_rule(positions, status, reached):
        stalled = np.flatnonzero(np.asarray(status) == STALLED)
        if stalled.size == 0:
            return {}
        plan = grid_plan(spec, walls, None, np.asarray(positions, np.float32), goal, 8, smooth=True, margin=0)
        replanned.append(len(stalled))
        return {int(i): plan["waypoints"][i, :plan["n_waypoints"][i]].copy() for i in stalled if plan["status"][i] == R.PLANNED}
    runs = []
    for cb in (planner.callback(goal), by_the_rule):
        runs.append(follow_with_replanning(e, _env("point", 32), start, first["waypoints"], cb, horizon=20, rounds=3, leg_steps=7,
                                           n_waypoints=first["n_waypoints"], seed=1, walls=walls))
    a, b = runs
    assert replanned and sum(replanned) > 0, "a leg budget of 7 steps stalls robots: the loop must have replanned some"
    assert a["state"].step0 == b["state"].step0 == 60
    for k in ("round_status", "status", "reached", "steps", "final_distance"):
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k    # (bytes: a robot without a plan has a NaN distance)
    assert np.array_equal(a["state"].n_waypoints, b["state"].n_waypoints)
    assert a["state"].waypoints.view(np.uint32).tobytes() == b["state"].waypoints.view(np.uint32).tobytes()
    assert np.array_equal(np.asarray(a["state"].positions), np.asarray(b["state"].positions))
    e.close()
