"""GPU: walls on the device (mobrob_ppo_follow_waypoints_walls; `walls=` on PPOEngine.follow_waypoints, DeviceGoalVecEnv.follow
and mobrob_amd.waypoints): n = 24 robots (a full tile of k_goal64_tile and a half one), K = 2, T = 60 steps, the hand-built
go-to-goal 2x64 actor of the other run tests, deterministic actions, on the tile and forced onto the per-step path.

Walls change no dynamics, so the scenes are built from a run without walls: a box of half-thickness 1e-4 across the midpoint of a
chosen robot's chosen step (a crossing with both ends clear), a box whose signed distance at the end of another step lies inside
(0, radius) (a contact without a crossing), far boxes.  M = 0, 5, 9 walls: uneven quarters.  Teacher forcing folds
goal_rules.wall_fold over the call's own positions (path_stride = 1: record r is the position after r steps, so records t and
t + 1 are the ends of step t) and must reproduce wall_out bit for bit."""
import numpy as np
import pytest

from mobrob_amd.envs.goal_rules import WALL_START, Hazards, MovingHazards, Schedule, Teams, Walls, wall_check, wall_fold
from mobrob_amd.waypoints import FollowState, follow_waypoints, wall_result
from tests.test_hazards_gpu import _go_to_goal
from tests.util import EVAL_CASES as CASES, _engine, _env, _snapshot, persistent_env  # noqa: F401

pytestmark = pytest.mark.gpu

N, K, T, RADIUS = 24, 2, 60, 0.12
PATHS = [CASES[1], ("point64_perstep", "point", dict(pi=(64, 64), vf=(64, 64)), "0", False)]
PATH_IDS = ["tile", "perstep"]
CARRIED = ("state", "robot", "arrival", "leg_used", "status", "hazard", "team", "sched", "release", "home", "wall", "step0")
WALL_KEYS = tuple(wall_result(FollowState(np.zeros((1, 2)), np.zeros((1, 1, 2)), walls=True)))


def _job(P):
    rng = np.random.default_rng(11)
    start = rng.uniform(-1.5, 1.5, (N, P)).astype(np.float32)
    wp = rng.uniform(-1.5, 1.5, (N, K, P)).astype(np.float32)
    nw = np.full(N, K, np.int32)
    nw[5], nw[19] = 0, 1                                  # a robot that never steps, one with a single waypoint
    return start, wp, nw


def _setup(case, persistent_env):
    name, robot, kw, pe, expect_persistent = case
    persistent_env(pe)
    e, _ = _engine(robot, kw)
    env = _env(robot, N)
    _go_to_goal(e, env)
    return e, env, expect_persistent


def _base(e, env, **kw):
    """the run without walls: its positions are what the scenes are built from"""
    start, wp, nw = _job(env.pos_dim)
    return env.follow(e, max_steps=T, seed=3, path_stride=1, trace=(N, T), resume=FollowState(start, wp, nw, pos_dim=env.pos_dim, **kw))


def _segments(r):
    """-> pre [T][N][2], post [T][N][2], stepped [T][N] of a call with path_stride = 1 and a full trace"""
    xy = np.zeros(r["path"].shape[:2] + (2,), np.float32)
    xy[..., :min(r["path"].shape[2], 2)] = r["path"][..., :2]
    return xy[:-1], xy[1:], np.any(r["trace"] != 0, axis=2)


def _moving_step(pre, post, stepped, i, t):
    """the first step >= t in which robot i stepped and moved ten times the half-thickness (a robot at rest or on hold does not)"""
    ok = stepped[t:, i] & (np.abs(post[t:, i].astype(np.float64) - pre[t:, i]).max(axis=1) > 1e-3)
    assert ok.any(), f"robot {i} does not move from step {t} on"
    return t + int(np.argmax(ok))


def _crossing_box(pre, post, stepped, i, t):
    t = _moving_step(pre, post, stepped, i, t)
    a, p = pre[t, i].astype(np.float64), post[t, i].astype(np.float64)
    d = np.abs(p - a)
    half = (1e-4, 0.02) if d[0] >= d[1] else (0.02, 1e-4)   # thin across the larger component of the motion
    return [*(0.5 * (a + p)), *half]


def _contact_box(post, stepped, i, t):
    t = t + int(np.argmax(stepped[t:, i]))
    assert stepped[t, i]
    p = post[t, i].astype(np.float64)
    return [p[0], p[1] - 0.05 - 0.5 * RADIUS, 0.05, 0.05]   # its upper face is RADIUS / 2 below the robot


def _scene(base, M):
    pre, post, stepped = _segments(base)
    if M == 0:
        return np.zeros((0, 4))
    far = [[50.0, 50.0, 1.0, 1.0], [-40.0, 30.0, 0.5, 2.0], [0.0, -60.0, 3.0, 0.1]]
    boxes = [_crossing_box(pre, post, stepped, 3, 10), _contact_box(post, stepped, 7, 4)] + far
    if M == 9:                                            # the half tile as well, and more of both kinds
        boxes += [_crossing_box(pre, post, stepped, 17, 2), _contact_box(post, stepped, 20, 12), _crossing_box(pre, post, stepped, 22, 30),
                  _contact_box(post, stepped, 0, 26)]
    assert len(boxes) == M
    return np.array(boxes)


def _walls(base, M, **kw):
    return Walls(_scene(base, M), radius=RADIUS, cost=1.5, indicator=False, **kw)


def _same_state(a, b, why, skip=()):
    for f in CARRIED:
        x, y = getattr(a, f, None), getattr(b, f, None)
        if f not in skip and not (x is None and y is None):
            assert np.array_equal(x, y, equal_nan=True), (why, f)


def _same_outputs(a, b, why, skip=()):
    for k in a:
        if k in ("state", "persistent") or k in skip:
            continue
        assert np.array_equal(a[k], b[k], equal_nan=True), (why, k)


@pytest.mark.parametrize("M", [0, 5, 9])
@pytest.mark.parametrize("case", PATHS, ids=PATH_IDS)
def test_teacher_forcing_and_observational(case, M, persistent_env):
    e, env, expect_persistent = _setup(case, persistent_env)
    start, wp, nw = _job(env.pos_dim)
    base = _base(e, env)
    walls = _walls(base, M)
    pre, post, stepped = _segments(base)
    if M:                                                 # the constructed cases are what they are meant to be
        tc, tk = _moving_step(pre, post, stepped, 3, 10), 4 + int(np.argmax(stepped[4:, 7]))
        c = wall_check(pre[tc, 3], post[tc, 3], walls.rows(), RADIUS)
        ends = [wall_check(x, x, walls.rows()[:1]) for x in (pre[tc, 3], post[tc, 3])]        # radius 0: the signed distance itself
        assert c[3] and all(cl > 0 and not hit for _, cl, _, hit in ends)
        c = wall_check(pre[tk, 7], post[tk, 7], walls.rows()[1:2], RADIUS, indicator=False)
        assert c[0] > 0 and -RADIUS < c[1] < 0 and not c[3]
    r = env.follow(e, start, wp, nw, max_steps=T, seed=3, path_stride=1, trace=(N, T), walls=walls)
    assert r["persistent"] == expect_persistent
    want = wall_fold(np.tile(WALL_START, (N, 1)), pre, post, stepped, walls)
    print(f"{case[0]} M={M}: contact steps {want[:, 1].astype(int).tolist()} crossing steps {want[:, 5].astype(int).tolist()}")
    assert np.array_equal(r["state"].wall, want, equal_nan=True), (r["state"].wall, want)
    assert np.array_equal(want[5], WALL_START, equal_nan=True)
    if M:
        assert want[3, 5] >= 1 and want[7, 1] >= 1 and np.sum(want[:, 5] == 0) > N // 2
    else:
        assert np.all(np.isposinf(want[stepped.any(0), 3])) and np.all(want[:, 4] == -1)
    for k in WALL_KEYS:
        assert np.array_equal(r[k], wall_result(r["state"])[k], equal_nan=True)
    # observational: every other output is the call without walls
    _same_outputs(base, r, "walls change nothing else")
    _same_state(base["state"], r["state"], "walls change nothing else", skip=("wall",))
    e.close()


@pytest.mark.parametrize("case", PATHS, ids=PATH_IDS)
def test_shared_scene_against_per_robot_scenes(case, persistent_env):
    e, env, _ = _setup(case, persistent_env)
    start, wp, nw = _job(env.pos_dim)
    base = _base(e, env)
    boxes = _scene(base, 9)
    shared = env.follow(e, start, wp, nw, max_steps=T, seed=3, walls=Walls(boxes, radius=RADIUS, cost=1.5, indicator=False))
    # the same scene twice (padded to 11 rows, 9 in use) and an empty one for the robots of scene 2
    table = np.zeros((3, 11, 4))
    table[0, :9], table[1, :9] = boxes, boxes
    scene = (np.arange(N) % 2).astype(np.int32)
    per = env.follow(e, start, wp, nw, max_steps=T, seed=3,
                     walls=Walls(table, counts=[9, 9, 0], scene=scene, radius=RADIUS, cost=1.5, indicator=False))
    assert np.array_equal(shared["state"].wall, per["state"].wall, equal_nan=True) and np.any(shared["crossing_steps"] > 0)
    scene[3] = 2                                          # robot 3 sees no walls now
    none = env.follow(e, start, wp, nw, max_steps=T, seed=3,
                      walls=Walls(table, counts=[9, 9, 0], scene=scene, radius=RADIUS, cost=1.5, indicator=False))["state"].wall
    assert none[3, 5] == 0 and np.isposinf(none[3, 3]) and np.array_equal(np.delete(none, 3, 0), np.delete(per["state"].wall, 3, 0), equal_nan=True)
    e.close()


@pytest.mark.parametrize("case", PATHS, ids=PATH_IDS)
def test_split_runs(case, persistent_env):
    e, env, _ = _setup(case, persistent_env)
    start, wp, nw = _job(env.pos_dim)
    walls = _walls(_base(e, env), 9)
    one = env.follow(e, start, wp, nw, max_steps=T, seed=3, walls=walls)
    for split in ((25, 35), (1, 59)):
        r = env.follow(e, start, wp, nw, max_steps=split[0], seed=3, walls=walls)
        r = env.follow(e, max_steps=split[1], seed=3, walls=walls, resume=r["state"])
        _same_state(one["state"], r["state"], split)
    # a replan in between keeps the wall record, and the run goes on accounting on top of it
    mid = env.follow(e, start, wp, nw, max_steps=25, seed=3, walls=walls)["state"]
    kept = mid.wall.copy()
    mid.replan([3, 17], np.array([[0.5, 0.5]], np.float32)[:, :env.pos_dim] if env.pos_dim == 2 else np.full((1, env.pos_dim), 0.5, np.float32))
    assert np.array_equal(mid.wall, kept, equal_nan=True)
    after = env.follow(e, max_steps=35, seed=3, walls=walls, resume=mid, path_stride=1, trace=(N, 35))
    pre, post, stepped = _segments(after)
    assert np.array_equal(after["state"].wall, wall_fold(kept, pre, post, stepped, walls, step0=25), equal_nan=True)
    e.close()


def _hazards(kind):
    xy = np.array([[0.0, 0.0], [0.6, 0.5], [-0.7, 0.3]])
    if kind == "static":
        return Hazards(xy, [0.4, 0.3, 0.35], cost=1.5, indicator=False)
    return MovingHazards.circling(xy, 0.3, [0.4, 0.3, 0.35], 4, 2.0, cost=1.5, indicator=False, frame_steps=7, loop=True)


@pytest.mark.parametrize("with_", ["static", "frames", "teams", "schedule", "all"])
@pytest.mark.parametrize("case", PATHS, ids=PATH_IDS)
def test_composition(case, with_, persistent_env):
    e, env, _ = _setup(case, persistent_env)
    start, wp, nw = _job(env.pos_dim)
    kw = {}
    if with_ in ("static", "frames"):
        kw["hazards"] = _hazards(with_)
    if with_ in ("teams", "all"):
        kw["teams"] = Teams(4, 0.5, 2.0)
    if with_ in ("schedule", "all"):
        kw["schedule"] = Schedule(np.array([0, 20]) + 3 * (np.arange(N) % 4)[:, None])
    if with_ == "all":
        kw["hazards"] = _hazards("frames")
    first = FollowState(start, wp, nw, "hazards" in kw, env.pos_dim, "teams" in kw, kw.get("schedule"))   # a call of a run, as with walls
    plain = env.follow(e, max_steps=T, seed=3, path_stride=1, trace=(N, T), resume=first, **kw)
    walls = _walls(plain, 9)                              # (a schedule changes the motion: the scene is built from this run)
    r = env.follow(e, start, wp, nw, max_steps=T, seed=3, path_stride=1, trace=(N, T), walls=walls, **kw)
    _same_outputs(plain, r, with_)
    _same_state(plain["state"], r["state"], with_, skip=("wall",))
    pre, post, stepped = _segments(plain)
    assert np.array_equal(r["state"].wall, wall_fold(np.tile(WALL_START, (N, 1)), pre, post, stepped, walls), equal_nan=True)
    assert np.any(r["crossing_steps"] > 0) and np.any(r["contact_steps"] > 0)
    if with_ in ("static", "frames", "teams"):            # the motion is the walls-only run's: so is wall_out
        alone = env.follow(e, start, wp, nw, max_steps=T, seed=3, walls=walls)
        assert np.array_equal(alone["state"].wall, r["state"].wall, equal_nan=True)
    e.close()


def test_refusals(persistent_env):
    e, env, _ = _setup(PATHS[0], persistent_env)
    start, wp, nw = _job(env.pos_dim)
    good = Walls([[0.0, 0.0, 0.5, 0.5]], radius=RADIUS)

    def tampered(**kw):
        w = Walls([[0.0, 0.0, 0.5, 0.5], [1.0, 1.0, 0.1, 0.1]], scene=np.zeros(N, np.int32), radius=RADIUS)
        for k, v in kw.items():
            setattr(w, k, v)
        return w
    neg, nan = np.array([[[0, 0, 0.5, 0.5], [1, 1, -0.1, 0.1]]], np.float32), np.array([[[0, 0, 0.5, 0.5], [np.nan, 1, 0.1, 0.1]]], np.float32)
    scene_bad = np.zeros(N, np.int32)
    scene_bad[9] = 1
    for w, msg in ((tampered(table=neg), "box 1 of scene 0"), (tampered(table=nan), "box 1 of scene 0"),
                   (tampered(table=np.zeros((1, 1025, 4), np.float32), counts=np.array([1025], np.int32)), "max_walls must lie in 0 .. 1024"),
                   (tampered(scene=scene_bad), r"scene\[9\] = 1 outside 0 .. 0"), (tampered(counts=np.array([3], np.int32)), r"n_walls\[0\] = 3"),
                   (tampered(radius=-1.0), "radius must be finite"), (tampered(cost=float("nan")), "cost must be finite")):
        st = FollowState(start, wp, nw, pos_dim=env.pos_dim, walls=True)
        with pytest.raises(ValueError, match="follow: walls: .*" + msg):
            env.follow(e, max_steps=5, seed=3, walls=w, resume=st)
        assert np.array_equal(st.wall, np.tile(WALL_START, (N, 1)), equal_nan=True) and st.step0 == 0
    for col, v in ((0, -1.0), (1, 0.5), (2, 7.0), (3, 1.0), (4, 1.0), (5, 2.0), (6, -2.0)):   # a carried record no call returns
        st = FollowState(start, wp, nw, pos_dim=env.pos_dim, walls=True)
        st.wall[2, col] = v
        with pytest.raises(ValueError, match="follow: walls: carried wall record of robot 2"):
            env.follow(e, max_steps=5, seed=3, walls=good, resume=st)
    with pytest.raises(ValueError, match="evaluate: walls"):                                 # evaluation takes no walls, by name
        e.evaluate_goal_env(env.pos_dim, env.mix, n_robots=4, max_steps=5, walls=good)
    with pytest.raises(ValueError, match="walls in every call or in none"):
        env.follow(e, max_steps=5, seed=3, walls=good, resume=FollowState(start, wp, nw, pos_dim=env.pos_dim))
    ok = env.follow(e, start, wp, nw, max_steps=5, seed=3, walls=good)                       # the engine is as usable as before
    assert np.all(ok["steps"][nw > 0] == 5)
    e.close()


@pytest.mark.parametrize("case", PATHS, ids=PATH_IDS)
def test_training_untouched(case, persistent_env):
    from mobrob_amd.envs.vec_env import DeviceGoalVecEnv
    name, robot, kw, pe, _ = case
    persistent_env(pe)
    env_a = DeviceGoalVecEnv.for_robot(robot, 16, time_limit=40, seed=5)
    env_b = DeviceGoalVecEnv.for_robot(robot, 16, time_limit=40, seed=5)
    ea, _ = _engine(robot, kw, seed=7)
    eb, _ = _engine(robot, kw, seed=7)
    start, wp, nw = _job(env_b.pos_dim)
    walls = Walls(Walls.enclosure(2.0, 0.2), radius=RADIUS)
    state = FollowState(start, wp, nw, pos_dim=env_b.pos_dim, walls=True)
    for it in range(2):
        env_a.collect(ea)
        env_b.collect(eb)
        before = _snapshot(eb, stats=False)
        env_b.follow(eb, start, wp, nw, max_steps=T, seed=it, walls=walls, trace=(4, 10), hazards=_hazards("static"))
        state = env_b.follow(eb, max_steps=13, seed=3, walls=walls, resume=state)["state"]
        sa, sb = _snapshot(ea, stats=False), _snapshot(eb, stats=False)
        for k in sa:
            assert np.array_equal(sa[k], sb[k]) and np.array_equal(before[k], sb[k]), f"iteration {it}: {k} differs"
        ea.train()
        eb.train()
        assert np.array_equal(ea.get_flat_params(), eb.get_flat_params())
    assert state.step0 == 26 and np.any(state.wall[:, 1] > 0)
    ea.close()
    eb.close()


def test_waypoints_module_takes_walls_on_the_device(persistent_env):
    e, env, _ = _setup(PATHS[0], persistent_env)
    start, wp, nw = _job(env.pos_dim)
    walls = Walls(Walls.enclosure(2.0, 0.2), radius=RADIUS)
    a = follow_waypoints(e, env, start, wp, nw, max_steps=30, seed=3, walls=walls)
    b = follow_waypoints(e, env, max_steps=30, seed=3, walls=walls, state=a["state"])
    one = env.follow(e, start, wp, nw, max_steps=60, seed=3, walls=walls)
    assert np.array_equal(b["state"].wall, one["state"].wall, equal_nan=True) and np.any(one["contact_steps"] > 0)
    e.close()
