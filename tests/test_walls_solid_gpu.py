"""GPU: solid walls on the device (mobrob_ppo_follow_waypoints_solid; Walls(..., solid=True) on PPOEngine.follow_waypoints,
DeviceGoalVecEnv.follow and mobrob_amd.waypoints): the shapes of tests/test_walls_gpu.py -- n = 24 robots (a full tile of
k_goal64_tile and a half one, a robot without waypoints, one with a single waypoint), K = 2, T = 60, the hand-built go-to-goal
2x64 actor, deterministic actions, on the tile and forced onto the per-step path.

The scenes are built from the run WITHOUT walls, as there: a thin box across the midpoint of a chosen robot's chosen step, so that
robot really is blocked.  Teacher forcing: for every traced step goal_rules.goal_propose32 from the traced (position, velocity,
action), then goal_rules.wall_block, must give the next traced position and velocity and the path record bit for bit."""
import numpy as np
import pytest

from mobrob_amd.envs.goal_rules import (BLOCKED_START, WALL_START, Hazards, MovingHazards, Schedule, Teams, Walls, goal_propose32,
                                        team_fold, wall_block, wall_block_velocity, wall_blocked_fold, wall_fold)
from mobrob_amd.waypoints import FollowState, blocked_result, follow_waypoints
from tests.test_hazards_gpu import _go_to_goal
from tests.test_walls_gpu import (N, K, T, PATHS, PATH_IDS, _base, _crossing_box, _job, _same_outputs, _same_state, _segments,
                                  _setup)
from tests.util import persistent_env  # noqa: F401

pytestmark = pytest.mark.gpu

RADIUS = 0.04                                             # small against the robots' spacing: few robots meet another robot's box
BLOCKED = (3, 22, 12)                                     # robots that get a thin box across one of their steps
FAR = [[50.0, 50.0, 1.0, 1.0], [-40.0, 30.0, 0.5, 2.0], [0.0, -60.0, 3.0, 0.1]]
SOLID_SKIP = ("wall", "blocked")


def _scene(base, robots=BLOCKED, far=FAR):
    pre, post, stepped = _segments(base)
    return np.array([_crossing_box(pre, post, stepped, i, t) for i, t in zip(robots, (10, 30, 8))] + list(far))


def _solid(boxes, **kw):
    return Walls(boxes, radius=RADIUS, cost=1.5, indicator=False, solid=True, **kw)


def _teacher(r, env, walls, extra=0):
    """-> (code, inside, stepped) [T][N] of a traced call with path_stride = 1, every traced step checked bit for bit"""
    P, D, A = env.pos_dim, r["trace"].shape[2] - 9 - env.mix.shape[1] - 4 - extra, env.mix.shape[1]
    tr, path = r["trace"], r["path"]
    steps, n = tr.shape[:2]
    stepped = np.any(tr != 0, axis=2)
    pos, vel, act = tr[..., 0:3], tr[..., 3:6], tr[..., 9 + D:9 + D + A]
    prop, v = goal_propose32(pos, vel, act, env.mix, env.dt, env.extent, P)
    code, inside = np.zeros((steps, n), np.int64), np.zeros((steps, n), bool)
    for i in range(n):
        q, code[:, i], inside[:, i] = wall_block(pos[:, i, :2], prop[:, i, :2], walls.rows(i), walls.radius)
        want_pos = prop[:, i].copy()
        want_pos[:, :2] = q
        want_vel = wall_block_velocity(v[:, i], code[:, i])
        for t in np.flatnonzero(stepped[:, i]):
            assert np.array_equal(path[t + 1, i].view(np.uint32), want_pos[t].view(np.uint32)), (i, t, "path")
            if t + 1 < steps and stepped[t + 1, i]:
                assert np.array_equal(tr[t + 1, i, :P].view(np.uint32), want_pos[t].view(np.uint32)), (i, t, "pos")
                assert np.array_equal(tr[t + 1, i, 3:3 + P].view(np.uint32), want_vel[t].view(np.uint32)), (i, t, "vel")
        if stepped[:, i].any():                           # the robot's last step (T - 1, or the one it finished on): the carried state
            t = int(np.flatnonzero(stepped[:, i])[-1])
            carried = r["state"].state[i]
            assert np.array_equal(carried[:P].view(np.uint32), want_pos[t].view(np.uint32)), (i, t, "carried pos")
            assert np.array_equal(carried[3:3 + P].view(np.uint32), want_vel[t].view(np.uint32)), (i, t, "carried vel")
    return np.where(stepped, code, 0), inside & stepped, stepped


@pytest.mark.parametrize("case", PATHS, ids=PATH_IDS)
def test_teacher_forcing(case, persistent_env):
    e, env, expect_persistent = _setup(case, persistent_env)
    start, wp, nw = _job(env.pos_dim)
    base = _base(e, env)
    walls = _solid(_scene(base))
    r = env.follow(e, start, wp, nw, max_steps=T, seed=3, path_stride=1, trace=(N, T), walls=walls)
    assert r["persistent"] == expect_persistent
    code, inside, stepped = _teacher(r, env, walls)
    want = wall_blocked_fold(np.tile(BLOCKED_START, (N, 1)), code, inside, stepped)
    print(f"{case[0]}: blocked steps {want[:, 0].tolist()} stopped {want[:, 2].tolist()} inside {want[:, 3].tolist()}")
    assert np.array_equal(r["state"].blocked, want)
    for k, v in blocked_result(r["state"]).items():
        assert np.array_equal(r[k], v)
    pre, post, _ = _segments(r)
    assert np.array_equal(r["state"].wall, wall_fold(np.tile(WALL_START, (N, 1)), pre, post, stepped, walls), equal_nan=True)
    never = want[:, 0] == 0
    assert np.sum(~never) >= 3 and np.sum(never) > N // 2
    # a robot that is never blocked moves as it does without walls: every output is the base run's
    for k in base:
        if k not in ("state", "persistent", "trace", "path") and np.ndim(base[k]) >= 1 and len(base[k]) == N:
            assert np.array_equal(np.asarray(base[k])[never], np.asarray(r[k])[never], equal_nan=True), k
    assert np.array_equal(base["path"][:, never], r["path"][:, never]) and np.array_equal(base["trace"][:, never], r["trace"][:, never])
    for f in ("state", "robot", "arrival", "leg_used", "status"):
        assert np.array_equal(getattr(base["state"], f)[never], getattr(r["state"], f)[never], equal_nan=True), f
    # the guarantees, on the device's own output
    free = r["wall_inside_steps"] == 0
    ran = r["steps"] > 0
    assert np.all(r["crossing_steps"][free] == 0) and np.all(r["min_wall_clearance"][free & ran] > -1e-6)
    assert np.all(base["steps"][~never] > 0) and np.any(r["path"][-1, ~never] != base["path"][-1, ~never])
    e.close()


@pytest.mark.parametrize("case", PATHS, ids=PATH_IDS)
def test_no_walls_and_far_walls_are_the_observational_call(case, persistent_env):
    e, env, _ = _setup(case, persistent_env)
    start, wp, nw = _job(env.pos_dim)
    for boxes in (np.zeros((0, 4)), np.array(FAR)):
        a = env.follow(e, start, wp, nw, max_steps=T, seed=3, path_stride=1, trace=(N, T), walls=Walls(boxes, radius=RADIUS, cost=1.5, indicator=False))
        b = env.follow(e, start, wp, nw, max_steps=T, seed=3, path_stride=1, trace=(N, T), walls=_solid(boxes))
        _same_outputs(a, b, "nothing to block", skip=tuple(blocked_result(b["state"])))
        _same_state(a["state"], b["state"], "nothing to block")
        assert np.array_equal(b["state"].blocked, np.tile(BLOCKED_START, (N, 1))) and a["state"].blocked is None
    e.close()


@pytest.mark.parametrize("case", PATHS, ids=PATH_IDS)
def test_shared_scene_against_per_robot_scenes(case, persistent_env):
    e, env, _ = _setup(case, persistent_env)
    start, wp, nw = _job(env.pos_dim)
    boxes = _scene(_base(e, env))
    M = len(boxes)
    shared = env.follow(e, start, wp, nw, max_steps=T, seed=3, walls=_solid(boxes))
    table = np.zeros((3, M + 2, 4))
    table[0, :M], table[1, :M] = boxes, boxes
    scene = (np.arange(N) % 2).astype(np.int32)
    per = env.follow(e, start, wp, nw, max_steps=T, seed=3, walls=_solid(table, counts=[M, M, 0], scene=scene))
    _same_state(shared["state"], per["state"], "shared against per-robot scenes")
    assert np.any(shared["wall_blocked_steps"] > 0) and np.array_equal(shared["state"].blocked, per["state"].blocked)
    scene[3] = 2                                          # robot 3 sees no walls now: it is not blocked, the others are as before
    none = env.follow(e, start, wp, nw, max_steps=T, seed=3, walls=_solid(table, counts=[M, M, 0], scene=scene))["state"]
    assert np.array_equal(none.blocked[3], BLOCKED_START) and np.array_equal(np.delete(none.blocked, 3, 0), np.delete(per["state"].blocked, 3, 0))
    e.close()


@pytest.mark.parametrize("case", PATHS, ids=PATH_IDS)
def test_split_run_with_a_replan(case, persistent_env):
    e, env, _ = _setup(case, persistent_env)
    start, wp, nw = _job(env.pos_dim)
    walls = _solid(_scene(_base(e, env)))
    one = env.follow(e, start, wp, nw, max_steps=T, seed=3, walls=walls)
    r = env.follow(e, start, wp, nw, max_steps=25, seed=3, walls=walls)
    r = env.follow(e, max_steps=35, seed=3, walls=walls, resume=r["state"])
    _same_state(one["state"], r["state"], "25 + 35")
    assert np.array_equal(one["state"].blocked, r["state"].blocked) and np.any(r["state"].blocked[:, 0] > 0)
    # the same replan between the calls of two differently split runs: 25 + 35 against 25 + 10 + 25
    new = np.full((1, env.pos_dim), 0.5, np.float32)
    mids = [env.follow(e, start, wp, nw, max_steps=25, seed=3, walls=walls)["state"] for _ in range(2)]
    for m in mids:
        kept = m.blocked.copy()
        m.replan([3, 17], new)
        assert np.array_equal(m.blocked, kept)
    a = env.follow(e, max_steps=35, seed=3, walls=walls, resume=mids[0])
    b = env.follow(e, max_steps=10, seed=3, walls=walls, resume=mids[1])
    b = env.follow(e, max_steps=25, seed=3, walls=walls, resume=b["state"])
    _same_state(a["state"], b["state"], "replanned")
    assert np.array_equal(a["state"].blocked, b["state"].blocked)
    e.close()


@pytest.mark.parametrize("with_", ["static", "teams", "schedule"])
@pytest.mark.parametrize("case", PATHS, ids=PATH_IDS)
def test_composition(case, with_, persistent_env):
    e, env, _ = _setup(case, persistent_env)
    start, wp, nw = _job(env.pos_dim)
    kw, extra = {}, 0
    if with_ == "static":
        kw["hazards"], extra = Hazards(np.array([[0.0, 0.0], [0.6, 0.5], [-0.7, 0.3]]), [0.4, 0.3, 0.35], cost=1.5, indicator=False), 2
    if with_ == "teams":
        kw["teams"] = Teams(4, 0.5, 2.0)
    if with_ == "schedule":
        kw["schedule"] = Schedule(np.array([0, 20]) + 3 * (np.arange(N) % 4)[:, None])
    plain = env.follow(e, max_steps=T, seed=3, path_stride=1, trace=(N, T),
                       resume=FollowState(start, wp, nw, "hazards" in kw, env.pos_dim, "teams" in kw, kw.get("schedule")), **kw)
    pre, post, stepped = _segments(plain)
    boxes = _scene(plain)
    if with_ == "schedule":
        # a hold next to a wall: a robot that reaches waypoint 0 before waypoint 1 is released goes on towards waypoint 0 -- its
        # anchor -- while it holds.  A thin box where it stands at the end of its last hold step, across its way there, far enough
        # from where it arrived that the inflated box does not hold its arrival position: it must be blocked DURING the hold.
        rel1 = kw["schedule"].for_robots(N, K, start)[0][:, 1]
        arr0 = plain["arrival"][:, 0]
        held = None
        for i in range(N):
            if nw[i] == 2 and i not in BLOCKED and 0 < arr0[i] < rel1[i] - 1 and stepped[arr0[i]:rel1[i], i].all():
                a, b = post[arr0[i] - 1, i].astype(np.float64), post[rel1[i] - 1, i].astype(np.float64)
                d = np.abs(b - a)
                if d.max() > RADIUS + 0.03:
                    held = (i, int(arr0[i]), int(rel1[i]))
                    boxes = np.concatenate([boxes, [[*b, *((1e-4, 0.02) if d[0] >= d[1] else (0.02, 1e-4))]]])
                    break
        assert held is not None, "no robot moves far enough towards its anchor while it holds"
    walls = _solid(boxes)
    r = env.follow(e, start, wp, nw, max_steps=T, seed=3, path_stride=1, trace=(N, T), walls=walls, **kw)
    code, inside, stepped = _teacher(r, env, walls, extra)
    assert np.array_equal(r["state"].blocked, wall_blocked_fold(np.tile(BLOCKED_START, (N, 1)), code, inside, stepped))
    pre, post, _ = _segments(r)
    assert np.array_equal(r["state"].wall, wall_fold(np.tile(WALL_START, (N, 1)), pre, post, stepped, walls), equal_nan=True)
    assert np.any(r["wall_blocked_steps"] > 0)
    free = r["wall_inside_steps"] == 0
    assert np.all(r["crossing_steps"][free] == 0) and np.all(r["min_wall_clearance"][free & (r["steps"] > 0)] > -1e-6)
    if with_ == "teams":                                  # the team check sees the resolved positions
        xy = np.zeros((T, N, 2))
        xy[:] = r["path"][0, :, :2]
        for t in range(T):
            xy[t:, stepped[t]] = r["path"][t + 1, stepped[t], :2][None]
        want = team_fold(np.tile(np.array([0.0, 0.0, -1.0, np.nan, -1.0]), (N, 1)), xy, stepped, kw["teams"])
        assert np.array_equal(r["state"].team, want, equal_nan=True)
    if with_ == "schedule":
        i, t0, t1 = held
        assert r["arrival"][i, 0] == t0 and r["hold_steps"][i] >= t1 - t0             # it arrives as before, then holds
        assert np.any(code[t0:t1, i] != 0), "the robot is not blocked in a hold step"
        assert r["wall_inside_steps"][i] == 0 and r["crossing_steps"][i] == 0 and r["wall_first_blocked"][i] <= t1
    e.close()


@pytest.mark.parametrize("case", PATHS, ids=PATH_IDS)
def test_a_start_inside_an_inflated_box_leaves_it(case, persistent_env):
    e, env, _ = _setup(case, persistent_env)
    start, wp, nw = _job(env.pos_dim)
    # robot 2 starts 0.02 from the face of a wall (inside the box inflated by RADIUS), its only waypoint straight away from it,
    # its second one straight back through the wall
    start[2, :2], wp[2, 0, :2], wp[2, 1, :2] = (0.0, 0.0), (-0.6, 0.0), (1.0, 0.0)
    walls = _solid(np.array([[0.02 + 0.1, 0.0, 0.1, 2.5]] + FAR))   # its face at x = 0.02, the inflated one at 0.02 - RADIUS < 0
    r = env.follow(e, start, wp, nw, max_steps=T, seed=3, path_stride=1, trace=(N, T), walls=walls)
    _teacher(r, env, walls)
    x = r["path"][:, 2, 0]
    assert r["wall_inside_steps"][2] > 0 and r["arrival"][2, 0] > 0 and x.min() < -RADIUS
    after = x[int(r["arrival"][2, 0]):]
    assert r["wall_blocked_steps"][2] > 0 and np.all(after <= 0.02 - RADIUS + 1e-6) and r["reached"][2] == 1
    e.close()


def test_a_thousand_walls_in_a_shared_scene(persistent_env):
    e, env, _ = _setup(PATHS[0], persistent_env)
    start, wp, nw = _job(env.pos_dim)
    base = _base(e, env)
    real = _scene(base, far=[])
    rng = np.random.default_rng(1)
    boxes = np.concatenate([rng.uniform(20, 60, (1024, 2)), rng.uniform(0, 1, (1024, 2))], 1)
    at = np.array([0, 511, 1023])
    boxes[at] = real
    big = env.follow(e, start, wp, nw, max_steps=T, seed=3, walls=_solid(boxes))
    few = env.follow(e, start, wp, nw, max_steps=T, seed=3, walls=_solid(real))
    assert big["persistent"] and np.any(big["wall_blocked_steps"] > 0)
    _same_state(few["state"], big["state"], "M = 1024", skip=("wall",))
    assert np.array_equal(few["state"].blocked, big["state"].blocked)
    assert np.array_equal(np.delete(few["state"].wall, 4, 1), np.delete(big["state"].wall, 4, 1), equal_nan=True)   # (but for the wall's index)
    e.close()


def test_refusals(persistent_env):
    e, env, _ = _setup(PATHS[0], persistent_env)
    start, wp, nw = _job(env.pos_dim)
    good = _solid([[0.0, 0.0, 0.5, 0.5]])
    moving = MovingHazards.circling(np.array([[0.0, 0.0]]), 0.3, [0.4], 4, 2.0, frame_steps=7, loop=True)
    with pytest.raises(ValueError, match="solid"):
        env.follow(e, start, wp, nw, max_steps=5, seed=3, walls=good, hazards=moving)
    with pytest.raises(ValueError, match="solid"):
        follow_waypoints(e, env, start, wp, nw, max_steps=5, seed=3, walls=good, hazards=moving)
    with pytest.raises(ValueError, match="evaluate: walls"):
        e.evaluate_goal_env(env.pos_dim, env.mix, n_robots=4, max_steps=5, walls=good)
    with pytest.raises(ValueError, match="solid walls in every call or in none"):
        env.follow(e, max_steps=5, seed=3, walls=good, resume=FollowState(start, wp, nw, pos_dim=env.pos_dim, walls=True))
    with pytest.raises(ValueError, match="solid walls in every call or in none"):
        env.follow(e, max_steps=5, seed=3, walls=Walls(good.table[0], radius=RADIUS), resume=FollowState(start, wp, nw, pos_dim=env.pos_dim, walls=good))
    for col, v in ((0, -1), (0, 1), (1, 3), (2, 1), (3, 9)):   # a carried record no call returns
        st = FollowState(start, wp, nw, pos_dim=env.pos_dim, walls=good)
        st.blocked[2, col] = v
        with pytest.raises(ValueError, match="follow: solid: carried blocked record of robot 2"):
            env.follow(e, max_steps=5, seed=3, walls=good, resume=st)
    # a scene that does not fit LDS is refused as before (a shared scene of hazards and of walls at their maxima)
    hz = Hazards(np.zeros((1024, 2)) + 40.0, 0.1)
    huge = _solid(np.tile([[40.0, 40.0, 0.1, 0.1]], (1024, 1)))
    from mobrob_amd.waypoints import FollowState as _FS
    for walls in (huge, Walls(huge.table[0], radius=RADIUS)):                                # solid or not: the same answer
        st = _FS(start, wp, nw, True, env.pos_dim, walls=walls)
        try:
            env.follow(e, max_steps=2, seed=3, walls=walls, hazards=hz, resume=st)
            fits = True
        except ValueError as ex:
            assert "follow: walls: the tile kernel needs" in str(ex) and "bytes of LDS" in str(ex)
            fits = False
        assert walls.solid or fits == fitted
        fitted = fits
    ok = env.follow(e, start, wp, nw, max_steps=5, seed=3, walls=good)                       # the engine is as usable as before
    assert np.all(ok["steps"][nw > 0] == 5)
    e.close()
