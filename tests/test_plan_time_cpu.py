"""CPU: the rule of planning over time (goal_rules.grid_layer_frames, grid_occupancy_time, grid_time_field, grid_walk_time,
grid_path_time, grid_plan_time): moving hazards as layers of occupancy, waits as release steps.  Integers but for grid_occupancy's
floats, so nothing here has a tolerance."""
import heapq

import numpy as np
import pytest

from mobrob_amd.envs import goal_rules as R
from mobrob_amd.envs.goal_rules import GridSpec, Hazards, MovingHazards, Walls, grid_plan, grid_plan_time
from mobrob_amd.planning import GridPlanner
from mobrob_amd.waypoints import FINISHED, GOING, STALLED
from tests.plan_scenes import EXTENT, INFLATE, SCENE0, robots33, three_hazards, two_scenes
from tests.plan_time_scenes import FAR, circling33, gap_case, goal_sitter, same_time


def frozen(h3, frames):
    """three_hazards as a MovingHazards of `frames` equal frames"""
    loc = np.repeat(h3.table[:, None, :, :2].astype(np.float64), frames, axis=1)
    return MovingHazards(loc, size=h3.table[:, :, 2].astype(np.float64), counts=h3.counts, scene=h3.scene, frame_steps=2, loop=frames > 1)


@pytest.mark.parametrize("frames", [1, 3])
def test_equal_frames_give_the_static_plan_bit_for_bit(frames):
    scene, start, goal = robots33()
    spec, walls, h3 = GridSpec(EXTENT, 32, INFLATE), two_scenes(scene), three_hazards(scene)
    ref = grid_plan(spec, walls, h3, start, goal, 4)
    got = grid_plan_time(spec, walls, frozen(h3, frames), start, goal, 4, step0=3, layer_steps=5, layers=6)
    same_time(got, ref, ("waypoints", "n_waypoints", "count", "status", "cost", "field_of", "field_goal_cell", "field_scene"))
    assert got["fields"].shape == (len(ref["fields"]), 7, 32, 32) and got["occupancy"].shape == (2, 7, 32, 32)
    for t in range(7):
        assert np.array_equal(got["fields"][:, t], ref["fields"]) and np.array_equal(got["occupancy"][:, t], ref["occupancy"])
    assert not got["waits"].any() and not got["release"].any()
    assert set(ref["status"].tolist()) == {R.PLANNED, R.UNREACHABLE, R.TRUNCATED}
    planned = ref["status"] != R.UNREACHABLE
    assert np.all(got["arrive"][~planned] == 0) and np.all(got["leave"][:, 0] == 0)


@pytest.mark.parametrize("loop", [False, True])
@pytest.mark.parametrize("frame_steps,layer_steps", [(7, 3), (5, 5), (3, 7), (2, 40)])
@pytest.mark.parametrize("step0", [0, 11])
def test_layer_frames_equal_a_step_by_step_enumeration(loop, frame_steps, layer_steps, step0):
    F, T = 6, 9                                    # the windows straddle the last frame: (T + 1) * layer_steps > F * frame_steps
    hz = MovingHazards(np.zeros((F, 1, 2)), frame_steps=frame_steps, loop=loop)
    first, number = R.grid_layer_frames(hz, step0, layer_steps, T)
    assert first.dtype == number.dtype == np.int32 and first.shape == number.shape == (T + 1,)
    for t in range(T + 1):
        run = [(int(first[t]) + j) % F for j in range(int(number[t]))]
        if t < T:
            steps = range(step0 + t * layer_steps, step0 + (t + 1) * layer_steps)
            want = []
            for g in steps:                        # distinct, in the order of the steps
                if hz.frame_index(g) not in want:
                    want.append(hz.frame_index(g))
            assert run == want, (t, run, want)
        else:
            want = set(range(F)) if loop else set(range(hz.frame_index(step0 + T * layer_steps), F))
            assert set(run) == want and len(run) == len(want)


def test_the_gap_scenario_waits_twice_and_hands_out_one_release_step():
    spec, walls, hz, start, goal = gap_case()
    p = grid_plan_time(spec, walls, hz, start, goal, 4, step0=0, layer_steps=10, layers=8)
    cells, acts, status = R.grid_walk_time(p["fields"][0], p["occupancy"][0], spec, start[0], goal[0])
    E, W = 0, R.PLAN_WAIT_ACTION
    assert status == R.PLANNED and acts == [E, E, W, W, E, E, E, E, E]
    assert p["cost"][0] == 43 == 7 * R.PLAN_STEP + 2 * R.PLAN_WAIT and p["count"][0] == 2 and p["status"][0] == R.PLANNED
    assert p["waits"].tolist() == [[0, 2, 0, 0]] and p["leave"].tolist() == [[0, 4, 0, 0]] and p["arrive"].tolist() == [9]
    assert p["release"].tolist() == [[0, 40, 0, 0]] and p["release"].dtype == np.int32
    assert np.array_equal(p["waypoints"][0, 0], np.float32([spec.centre(14), spec.centre(19)])) and np.array_equal(p["waypoints"][0, 1], goal[0])
    assert R.PLAN_WAIT < R.PLAN_STEP
    # started later, the hazard leaves sooner: one wait from step 25 on (layers 25 .. 34, 35 .. 44: blocked in the first two only)
    q = grid_plan_time(spec, walls, hz, start, goal, 4, step0=25, layer_steps=10, layers=8)
    assert q["waits"].tolist() == [[0, 0, 0, 0]] and q["cost"][0] == 35   # two moves pass before the gap is needed: free by then
    r = grid_plan_time(spec, walls, hz, start[:, :2] + np.float32([0.25, 0]), goal, 4, step0=25, layer_steps=10, layers=8)
    assert r["waits"].tolist() == [[2, 0, 0, 0]] and r["release"].tolist() == [[45, 0, 0, 0]] and r["count"][0] == 1   # waits at the start: the hold at home


def forward_dijkstra(occ, spec, start_xy, goal_xy):
    """min cost from (start cell, layer 0) to the goal cell over (cell, layer) states, forwards -- not the rule's backward sweep"""
    T, G = occ.shape[0] - 1, occ.shape[1]
    sx, sy = (int(v) for v in spec.cell_of(np.asarray(start_xy, np.float32)))
    gx, gy = (int(v) for v in spec.cell_of(np.asarray(goal_xy, np.float32)))
    if occ[0, sy, sx]:
        return -1
    best, heap = {(0, sx, sy): 0}, [(0, 0, sx, sy)]
    while heap:
        c, t, ix, iy = heapq.heappop(heap)
        if c != best[(t, ix, iy)]:
            continue
        if (ix, iy) == (gx, gy):
            return c
        t1 = min(t + 1, T)
        steps = [(ix + dx, iy + dy, R.PLAN_STEP if k < 4 else R.PLAN_DIAG) for k, (dx, dy) in enumerate(R.PLAN_DIRS)
                 if R.plan_move_ok(occ[t], ix, iy, k)]
        if t < T:
            steps.append((ix, iy, R.PLAN_WAIT))
        for jx, jy, w in steps:
            if occ[t1, jy, jx]:
                continue
            if c + w < best.get((t1, jx, jy), 1 << 30):
                best[(t1, jx, jy)] = c + w
                heapq.heappush(heap, (c + w, t1, jx, jy))
    return -1


def random_scene(seed):
    rng = np.random.default_rng(seed)
    boxes = np.concatenate([Walls.enclosure(3.6, 0.2), np.column_stack([rng.uniform(-1.3, 1.3, (5, 2)), rng.uniform(0.02, 0.35, (5, 2))])])
    centres = rng.uniform(-1.2, 1.2, (4, 2))
    hz = MovingHazards.circling(centres, travel=0.4, size=0.12, n_frames=10, dt=2 * np.pi / 10, frame_steps=int(rng.integers(2, 7)),
                                loop=bool(seed % 2))
    n = 12
    return (GridSpec(EXTENT, 32, INFLATE), Walls(boxes, radius=0.05), hz, rng.uniform(-1.5, 1.5, (n, 2)).astype(np.float32),
            rng.uniform(-1.5, 1.5, (n, 2)).astype(np.float32), int(rng.integers(0, 30)), int(rng.integers(2, 9)), int(rng.integers(3, 13)))


@pytest.fixture(scope="module", params=[1, 2, 3, 4])
def random_plan(request):
    spec, walls, hz, start, goal, step0, layer_steps, layers = random_scene(request.param)
    return spec, walls, hz, start, goal, step0, layer_steps, layers, grid_plan_time(spec, walls, hz, start, goal, 6, step0, layer_steps, layers)


def test_cost_equals_an_independent_forward_dijkstra(random_plan):
    spec, walls, hz, start, goal, step0, layer_steps, layers, p = random_plan
    assert np.any(p["status"] != R.UNREACHABLE)
    for i in range(len(start)):
        want = forward_dijkstra(p["occupancy"][0], spec, start[i], goal[i])
        assert p["cost"][i] == want, (i, p["cost"][i], want)
        assert (p["status"][i] == R.UNREACHABLE) == (want < 0)


def replay(p, spec, start, goal, K):
    """every walk again, action by action: the cells plan_move_ok needs are free in that layer's map, the target is free in the next
    one, the costs sum to the plan's, and the waypoints, waits, leave and arrive are what the actions say"""
    T = p["occupancy"].shape[1] - 1
    walked = waited = 0
    for i in range(len(start)):
        f = p["field_of"][i]
        occ, d = p["occupancy"][p["field_scene"][f]], p["fields"][f]
        cells, acts, status = R.grid_walk_time(d, occ, spec, start[i], goal[i])
        assert (status == R.UNREACHABLE) == (p["status"][i] == R.UNREACHABLE)
        if status == R.UNREACHABLE:
            assert p["count"][i] == 0 and p["cost"][i] == -1 and p["arrive"][i] == 0 and not p["waits"][i].any()
            continue
        total = 0
        for a, k in enumerate(acts):
            t, (ix, iy) = min(a, T), cells[a]
            assert not occ[t, iy, ix]
            if k == R.PLAN_WAIT_ACTION:
                assert a < T and cells[a + 1] == (ix, iy) and not occ[t + 1, iy, ix]
                total += R.PLAN_WAIT
            else:
                assert R.plan_move_ok(occ[t], ix, iy, k) and cells[a + 1] == (ix + R.PLAN_DIRS[k][0], iy + R.PLAN_DIRS[k][1])
                assert not occ[min(t + 1, T), cells[a + 1][1], cells[a + 1][0]]
                total += R.PLAN_STEP if k < 4 else R.PLAN_DIAG
        assert total == p["cost"][i] and len(acts) == p["arrive"][i] and cells[-1] == tuple(int(v) for v in spec.cell_of(goal[i]))
        moves = [a for a, k in enumerate(acts) if k != R.PLAN_WAIT_ACTION]
        anchors = [(0, moves[0] if moves else 0)]  # (actions before the walk stood in the anchor, actions before the move that leaves it)
        for j, a in enumerate(moves[1:], 1):
            if acts[a] != acts[moves[j - 1]] or a - moves[j - 1] > 1:
                anchors.append((moves[j - 1] + 1, a))
        assert p["count"][i] == len(anchors)
        for k, (enter, leave) in enumerate(anchors[:K]):
            assert (p["waits"][i, k], p["leave"][i, k]) == (leave - enter, leave), (i, k)
            assert p["release"][i, k] == (0 if leave == enter else p["step0"] + leave * p["layer_steps"])
            if k:
                assert np.array_equal(p["waypoints"][i, k - 1], np.float32([spec.centre(cells[leave][0]), spec.centre(cells[leave][1])]))
        walked += len(moves)
        waited += len(acts) - len(moves)
    return walked, waited


def test_every_walk_replays_in_free_cells_of_its_layers(random_plan):
    spec, walls, hz, start, goal, step0, layer_steps, layers, p = random_plan
    walked, _ = replay(dict(p, step0=step0, layer_steps=layer_steps), spec, start, goal, 6)
    assert walked > 0


def test_walks_of_the_circling_scene_and_the_gap_replay_with_waits():
    spec, walls, hz, scene, start, goal = circling33()
    p = grid_plan_time(spec, walls, hz, start, goal, 4, step0=7, layer_steps=10, layers=8)
    replay(dict(p, step0=7, layer_steps=10), spec, start, goal, 4)
    spec, walls, hz, start, goal = gap_case()
    p = grid_plan_time(spec, walls, hz, start, goal, 4, step0=0, layer_steps=10, layers=8)
    assert replay(dict(p, step0=0, layer_steps=10), spec, start, goal, 4) == (7, 2)


def test_every_disc_centre_of_a_layers_window_is_blocked_in_that_layer(random_plan):
    spec, walls, hz, start, goal, step0, layer_steps, layers, p = random_plan
    assert float(spec.h) / np.sqrt(2) < 0.12 + INFLATE       # a disc covers the centre of the cell its own centre lies in
    for t in range(layers):
        for g in range(step0 + t * layer_steps, step0 + (t + 1) * layer_steps):
            for x, y, _ in hz.rows(0, g):
                ix, iy = spec.cell_of(np.float32([x, y]))
                assert p["occupancy"][0, t, iy, ix], (t, g, x, y)
    for g in range(step0 + layers * layer_steps, step0 + layers * layer_steps + 2 * hz.n_frames * hz.frame_steps):
        for x, y, _ in hz.rows(0, g):
            ix, iy = spec.cell_of(np.float32([x, y]))
            assert p["occupancy"][0, layers, iy, ix], ("tail", g, x, y)


def test_a_goal_that_frees_up_is_waited_for_and_a_goal_blocked_in_the_tail_is_unreachable():
    spec, hz, start, goal = goal_sitter(stay=40)
    p = grid_plan_time(spec, None, hz, start, goal, 4, step0=0, layer_steps=10, layers=8)
    gx, gy = spec.cell_of(goal[0])
    assert p["occupancy"][0, :4, gy, gx].all() and not p["occupancy"][0, 4:, gy, gx].any()
    assert p["status"][0] == R.PLANNED and p["cost"][0] >= 0 and np.all(p["fields"][0, :4, gy, gx] == -1) and np.all(p["fields"][0, 4:, gy, gx] == 0)
    assert p["arrive"][0] == 10 and p["cost"][0] == 10 * R.PLAN_STEP    # ten columns away: the hazard is gone before the robot is there
    near = goal - np.float32([3 * float(spec.h), 0])                    # three columns away: there before the disc leaves, so it waits
    q = grid_plan_time(spec, None, hz, near, goal, 4, step0=0, layer_steps=10, layers=8)
    assert q["status"][0] == R.PLANNED and q["waits"].sum() >= 1 and q["release"].max() == 40       # the last move is made in layer 4
    assert q["cost"][0] == forward_dijkstra(q["occupancy"][0], spec, near[0], goal[0]) < 3 * R.PLAN_STEP + 3 * R.PLAN_WAIT
    assert replay(dict(q, step0=0, layer_steps=10), spec, near, goal, 4)[1] == q["waits"].sum()
    short = grid_plan_time(spec, None, hz, start, goal, 4, step0=0, layer_steps=10, layers=2)   # the tail starts at step 20: still blocked
    assert short["occupancy"][0, 2, gy, gx] and short["status"][0] == R.UNREACHABLE and short["count"][0] == 0 and short["cost"][0] == -1


def test_refusals_name_the_argument():
    spec, walls, hz, start, goal = gap_case()
    for kw, word in ((dict(layers=0), "layers"), (dict(layers=257), "layers"), (dict(layer_steps=0), "layer_steps"), (dict(step0=-1), "step0"),
                     (dict(layers=2.0), "layers"), (dict(layer_steps=True), "layer_steps"),
                     (dict(step0=2 ** 31 - 90, layer_steps=10, layers=8), "fit an int32")):
        args = dict(step0=0, layer_steps=10, layers=8)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            grid_plan_time(spec, walls, hz, start, goal, 4, **args)
    assert R.plan_time_check(2 ** 31 - 1 - 90, 10, 8) == (2 ** 31 - 91, 10, 8)          # the last step that fits
    with pytest.raises(TypeError, match="MovingHazards"):
        grid_plan_time(spec, walls, Hazards([[0.0, 0.0]]), start, goal, 4, 0, 10, 8)
    with pytest.raises(TypeError, match="moving hazards"):
        R.plan_scene(walls, hz)                                                        # the static rule keeps refusing them
    with pytest.raises(ValueError, match="scenes"):
        grid_plan_time(spec, two_scenes(np.zeros(1, int)), hz, start, goal, 4, 0, 10, 8)
    assert R.PLAN_TIME_MAX_BYTES == 256 << 20 and R.PLAN_LAYERS_MAX == 256
    n = 64                                                                              # 64 fields x 257 layers x 128 x 128 x 4 bytes = 1028 MiB
    big_goal = np.column_stack([np.linspace(-1.5, 1.5, n), np.zeros(n)]).astype(np.float32)
    with pytest.raises(ValueError, match="exceed the cap"):
        grid_plan_time(GridSpec(EXTENT, 128), None, hz, np.zeros((n, 2), np.float32), big_goal, 4, 0, 1, 256)
    with pytest.raises(ValueError, match="max_waypoints"):
        R.grid_path_time(np.zeros((2, 32, 32), np.int32), np.zeros((2, 32, 32), bool), spec, [0, 0], [0, 0], 0)


def test_grid_planner_on_an_env_name_plans_in_time_and_hands_out_a_schedule():
    spec, walls, hz, start, goal = gap_case()
    planner = GridPlanner("point", walls=walls, hazards=hz, cells=32, inflate=INFLATE, max_waypoints=4, extent=EXTENT, layer_steps=10, layers=8)
    got = planner.plan(start, goal, want_occupancy=True, want_fields=True)
    same_time(got, grid_plan_time(spec, walls, hz, start, goal, 4, 0, 10, 8))
    assert isinstance(got["schedule"], R.Schedule) and got["schedule"].release.tolist() == [[0, 40, 0, 0]]
    assert np.array_equal(got["schedule"].home, start) and not got["fields_reused"] and got["smoothed"] is False and got["moves"] is None
    assert planner.plan(start, goal, 25)["cost"][0] == 35
    assert GridPlanner("point", walls=walls, hazards=hz, cells=32, extent=EXTENT, layer_steps=10).layers == 64
    two = GridPlanner("point", walls=walls, hazards=hz, cells=32, inflate=INFLATE, max_waypoints=1, extent=EXTENT, layer_steps=10, layers=8)
    assert two.plan(start, goal)["status"][0] == R.TRUNCATED
    grown = two.plan(start, goal, grow=True)
    assert grown["status"][0] == R.PLANNED and grown["release"].tolist() == [[0, 40]]
    with pytest.raises(ValueError, match="layer_steps"):
        GridPlanner("point", walls=walls, hazards=hz, cells=32, extent=EXTENT)
    with pytest.raises(ValueError, match="smooth"):
        GridPlanner("point", walls=walls, hazards=hz, cells=32, extent=EXTENT, layer_steps=10, smooth=True)
    with pytest.raises(ValueError, match="smooth"):
        planner.plan(start, goal, smooth=True)
    with pytest.raises(ValueError, match="horizon"):
        planner.callback(goal)
    with pytest.raises(ValueError, match="layer_steps"):
        GridPlanner("point", walls=walls, cells=32, extent=EXTENT, layer_steps=10)
    static = GridPlanner("point", walls=walls, cells=32, extent=EXTENT)
    with pytest.raises(ValueError, match="horizon"):
        static.callback(goal, horizon=10)
    with pytest.raises(ValueError, match="step0"):
        static.plan(start, goal, 5)


def test_timed_callback_counts_its_calls_and_returns_release_steps():
    spec, walls, hz, start, goal = gap_case()
    start4, goal4 = np.repeat(start, 4, axis=0), np.repeat(goal, 4, axis=0)
    planner = GridPlanner("point", walls=walls, hazards=hz, cells=32, inflate=INFLATE, max_waypoints=4, extent=EXTENT, layer_steps=10, layers=8)
    cb = planner.callback(goal4, horizon=5)
    status = np.array([GOING, STALLED, FINISHED, STALLED])
    assert cb(start4, np.array([GOING] * 4), np.zeros(4, int)) == {} and cb.calls == 1 and cb.last is None
    new = cb(start4, status, np.zeros(4, int))                      # call 2: after 10 steps; layers 10 .. 19, 20 .. 29, 30 .. 39 are blocked: E, E, one wait
    assert sorted(new) == [1, 3] and cb.calls == 2
    ref = grid_plan_time(spec, walls, hz, start4, goal4, 4, 10, 10, 8)
    for i in (1, 3):
        w, rel = new[i]
        assert w.view(np.uint32).tobytes() == ref["waypoints"][i, :ref["count"][i]].view(np.uint32).tobytes()
        assert rel.tolist() == ref["release"][i, :ref["count"][i]].tolist() == [0, 40]
    for _ in range(6):
        cb(start4, status, np.zeros(4, int))
    assert cb.calls == 8 and not cb.last["waits"].any()             # after 40 steps the gap is free


def test_cli_plans_in_time_with_hazard_frames(capsys, tmp_path):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mod = importlib.util.spec_from_file_location("follow_cli_time", os.path.join(root, "examples", "follow.py"))
    cli = importlib.util.module_from_spec(mod)
    mod.loader.exec_module(cli)

    class Wander:
        def predict(self, obs, deterministic=True):
            return np.array([0.6, 0.3]), None
    frames = np.array([[[0.0, 0.4375, 0.1]], [list(FAR) + [0.1]]])
    r = cli.follow("point", "ppo", None, 4, max_steps=30, host=True, seed=3, policy=Wander(), walls=np.array([[0.0, -0.65, 0.02, 0.95]]),
                   arena=True, goal=[0.7, 0.4], plan_cells=32, horizon=10, leg_steps=4, hazard_frames=frames, frame_steps=40,
                   plan_layer_steps=10, plan_layers=8)
    out = capsys.readouterr().out.splitlines()
    assert out[0].startswith("planned rate: ") and r["state"].release is not None and r["state"].release.shape[0] == 4
