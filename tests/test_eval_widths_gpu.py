"""GPU: the one-launch evaluation tiles at every observation width, with an actor that reads every feature.

k_goal64_tile<DP, Task> is compiled for DP = 16, 32, 48, 64 and every task; the other GPU tests of the family launch it with doggo
(64) and point (16) only, and their wall, team and hazard runs use a hand-built actor whose W1 reads the first P features.  Here
car (D = 26: DP = 32), turtlebot3 (43: 48) and drone (12: 16, but A = 18 -- the second head block -- and P = 3) run every task
with the random actor of tests.util._engine (every feature below D carries weight: tests/test_eval_widths_cpu.py shows that a
dropped or misplaced layer-1 k-step, or a dropped head block, leaves the bound on these very weights); doggo joins for the wall
tasks, which had run point only.  k_goal256_tile runs car and turtlebot3: 8 and 12 layer-1 k-steps.

Shapes: 24 robots (a full 16-robot tile and a half one), K = 2 waypoints, 60 steps, path_stride 1, full trace; evaluations with
time_limit 40.  The job is tests.eval_widths.job (tests.test_follow_gpu._paths puts every waypoint of a K = 2 job next to the start:
no robot would be left under way).  Scenes are built from the call's own wall-free run, as in tests/test_walls_gpu.py.

Bounds are the project's own: 1e-5 * max(1, max|want|) for the traced action against the float64 oracle on the traced
observations, 2e-6 for the reward, test_hazards_gpu's TOL for costs and clearances, bit for bit for every rule fold and for runs
split into calls.  Measured action errors on the MI355X (printed by the tests):
  k_goal64_tile   car 4.2e-7 (evaluation) / 4.2e-7 (follow), turtlebot3 3.9e-7 / 3.0e-7, drone 6.3e-7 / 6.0e-7, doggo (walls) 4.2e-7
  k_goal256_tile  car 5.7e-7 / 6.3e-7, turtlebot3 4.8e-7 / 4.8e-7
The hazard, team, wall and solid-wall tasks give the figures of the task they wrap on the same observations."""
import numpy as np
import pytest

from mobrob_amd.envs.goal_rules import (BLOCKED_START, SCHED_START, TEAM_START, WALL_START, Hazards, MovingHazards, Schedule, Teams,
                                        Walls, schedule_fold, team_fold, wall_blocked_fold, wall_fold)
from mobrob_amd.waypoints import FollowState, blocked_result
from oracle import ppo_oracle as O
from tests import eval_widths as W
from tests.eval_model import goal_advance, trace_fields
from tests.eval_widths import FOLLOW_SEED, K, N, T, TL
from tests.test_eval_tile256_gpu import _engine256, _same
from tests.test_follow_gpu import _check_trace
from tests.test_hazard_frames_gpu import _teacher_by_step
from tests.test_hazards_gpu import _recount, _teacher_check
from tests.test_walls_gpu import _contact_box, _crossing_box, _same_outputs, _same_state, _segments
from tests.test_walls_solid_gpu import _teacher
from tests.util import _engine, _env, persistent_env  # noqa: F401

pytestmark = pytest.mark.gpu

TILES = [(r, 64) for r in W.ROBOTS] + [("car", 256), ("turtlebot3", 256)]
TILE_IDS = [f"{r}{w}" for r, w in TILES]


def _make(robot, width):
    """the engine, with the weights tests/test_eval_widths_cpu.py examined"""
    e, p = _engine256(robot) if width == 256 else _engine(robot, W.KW64)
    want = W.host_params(robot, W.KW256 if width == 256 else W.KW64)
    assert list(p) == list(want) and all(np.array_equal(p[k], want[k]) for k in want)
    return e, p


def _actor_error(p, f, live, what):
    mean, _ = O.policy_outputs(p, f["obs"][live].astype(np.float32), activation="tanh")
    want = np.clip(mean, -1.0, 1.0)
    err, bound = float(np.max(np.abs(f["act"][live] - want))), 1e-5 * max(1.0, float(np.max(np.abs(want))))
    print(f"{what}: tile action error {err:.3e} against the float64 oracle, bound {bound:.3e}")
    assert err <= bound, (what, err, bound)


def _standing(path, stepped):
    """[T][N][2]: x, y of every robot after each step (a robot that did not step: where it stands)"""
    xy = np.zeros((T, N, 2))
    xy[:] = path[0, :, :2]
    for t in range(T):
        xy[t:, stepped[t]] = path[t + 1, stepped[t], :2][None]
    return xy


def _separation(path, stepped, size=4):
    """a separation in the widest gap between the teams' closest approaches: the teams below it conflict, those above never do"""
    xy = _standing(path, stepped)
    closest = []
    for g in range(N // size):
        m = xy[:, size * g:size * (g + 1)]
        d = np.linalg.norm(m[:, :, None] - m[:, None, :], axis=3) + np.where(np.eye(size, dtype=bool), np.inf, 0.0)[None]
        d = np.where(stepped[:, size * g:size * (g + 1), None], d, np.inf)
        closest.append(float(d.min()))
    closest = np.sort(closest)
    j = int(np.argmax(np.diff(closest)))
    assert closest[j + 1] - closest[j] > 1e-3, closest
    return 0.5 * float(closest[j] + closest[j + 1])


def _conflicts(r, size=4):
    """a team with conflict steps and a team without any"""
    per_team = r["conflict_steps"].reshape(N // size, size).sum(1)
    assert np.any(per_team > 0) and np.any(per_team == 0), per_team


def _hazards_on(path, rows, kind):
    """three hazards where the robots `rows` stand after step 9 (travel 0.2 < every size: they are charged in that step)"""
    cen = path[10, rows, :2].astype(np.float64)
    if kind == "static":
        return Hazards(cen, [0.3, 0.25, 0.35], cost=1.5, indicator=False)
    return MovingHazards.circling(cen, 0.2, [0.3, 0.25, 0.35], 4, 2.0, cost=1.0, indicator=kind == "frames", frame_steps=7, loop=True)


def _charged(r):
    """some hazard cost above 0, and a robot that ran and was never charged"""
    assert np.any(r["cost_sum"] > 0) and np.any((r["cost_sum"] == 0) & (r["steps"] > 0)), r["cost_sum"]


def _replay_evaluation(r, f, env, S, R):
    """tests/test_eval_gpu.py::test_teacher_forced_trace: the transitions and the sums over the trace"""
    P = env.pos_dim
    for t in range(S):
        pos2, vel2, rew, reached = goal_advance(f["pos"][t], f["vel"][t], f["goal"][t], f["act"][t], env.mix, P, env.dt,
                                                env.extent, extra_bonus=env.extra_bonus)
        assert np.max(np.abs(f["reward"][t] - rew)) <= 2e-6
        assert np.array_equal(f["reached"][t], reached)
        if t + 1 == S:
            break
        cont = ~(f["term"][t] | f["tr"][t])
        assert np.allclose(f["pos"][t + 1][cont, :P], pos2[cont], atol=1e-6)
        assert np.allclose(f["vel"][t + 1][cont, :P], vel2[cont], atol=1e-6)
        assert np.array_equal(f["goal"][t + 1][cont], f["goal"][t][cont])
        rch = f["term"][t]
        assert np.allclose(f["pos"][t + 1][rch, :P], pos2[rch], atol=1e-6)
        assert np.all(np.abs(f["goal"][t + 1][rch, :P]) <= env.extent)
        trc = f["tr"][t]
        assert np.all(np.abs(f["pos"][t + 1][trc, :P]) <= env.extent / 2)
        assert np.all(f["vel"][t + 1][trc] == 0.0)
    assert f["tr"].any(), "the run should truncate some episodes (time_limit 40 < 60 steps)"
    rew64 = f["reward"].astype(np.float64)
    for i in range(R):
        assert r["reward_sum"][i] == sum(float(x) for x in rew64[:, i])
        assert r["steps"][i] == S
        ends = np.nonzero(f["term"][:, i] | f["tr"][:, i])[0]
        assert r["episodes"][i] == len(ends)
        assert r["goals"][i] == int(f["reached"][:, i].sum())
        start = 0
        for k, end in enumerate(ends):
            ret = 0.0
            for x in rew64[start:end + 1, i]:
                ret += float(x)
            assert r["episode_returns"][i, k] == ret
            assert r["episode_lengths"][i, k] == end + 1 - start
            assert r["episode_success"][i, k] == float(f["reached"][end, i])
            start = end + 1


EVAL = dict(n_robots=N, max_steps=T, episodes=0, quota=np.full(N, 50, np.int32), trace=(N, T), seed=W.EVAL_SEED)


@pytest.mark.parametrize("robot,width", TILES, ids=TILE_IDS)
def test_evaluation(robot, width, persistent_env):
    """EvalTask at DP = 32, 48 and 16 with the wide head; k_goal256_tile at 8 and 12 layer-1 k-steps"""
    persistent_env(None)
    e, p = _make(robot, width)
    env = _env(robot, N, tl=TL)
    r = env.evaluate(e, **EVAL)
    assert r["persistent"] is True
    f = trace_fields(r["trace"], e.D, e.A)
    _actor_error(p, f, np.ones((T, N), bool), f"{robot} {width} evaluation")
    _replay_evaluation(r, f, env, T, N)
    e.close()


@pytest.mark.parametrize("kind", ["static", "frames"])
@pytest.mark.parametrize("robot", W.ROBOTS)
def test_evaluation_with_hazards(robot, kind, persistent_env):
    """the static and the framed hazard task around EvalTask (two more trace columns): the same actor bound, cost and clearance
    against goal_rules.hazard_cost as tests/test_hazards_gpu.py and tests/test_hazard_frames_gpu.py check them"""
    persistent_env(None)
    e, p = _make(robot, 64)
    env = _env(robot, N, tl=TL)
    D, A, Wd = e.D, e.A, 9 + e.D + e.A + 4
    base = env.evaluate(e, **EVAL)
    hz = _hazards_on(trace_fields(base["trace"], D, A)["pos"], [0, 9, 17], kind)
    r = env.evaluate(e, hazards=hz, **EVAL)
    assert base["persistent"] is True and r["persistent"] is True
    assert r["trace"].shape[2] == Wd + 2 and np.array_equal(base["trace"], r["trace"][:, :, :Wd])
    f = trace_fields(r["trace"], D, A)
    live = np.any(r["trace"][:, :, :Wd] != 0, axis=2)
    assert live.all() and f["tr"].any()
    _actor_error(p, f, live, f"{robot} 64 evaluation, {kind} hazards")
    nxt = np.zeros_like(live)                                 # the post-step position is the next row's state where no episode ended
    nxt[:-1] = live[:-1] & ~f["term"][:-1] & ~f["tr"][:-1]
    post = np.zeros((T, N, 2), np.float32)
    post[:-1] = f["pos"][1:, :, :2]
    cost, clear = r["trace"][:, :, Wd], r["trace"][:, :, Wd + 1]
    if kind == "static":
        cmp_, left = _teacher_check(cost, clear, post, nxt, lambda i: hz.rows(i), hz.cost, hz.indicator)
    else:
        cmp_, left = _teacher_by_step(cost, clear, post, nxt, hz)
    _recount(cost, live, r, N)
    print(f"{robot} {kind}: compared {cmp_} rows, left out {left}")
    assert cmp_ > 0 and left <= 0.001 * cmp_
    _charged(r)
    e.close()


@pytest.mark.parametrize("robot,width", TILES, ids=TILE_IDS)
def test_follow(robot, width, persistent_env):
    """FollowTask teacher-forced, then ResumeFollowTask with sampled actions: one 60-step call against three 20-step calls (drone's
    five noise groups for A = 18 and car's half group for A = 2 are the edges of eval_actions)"""
    persistent_env(None)
    e, p = _make(robot, width)
    env = _env(robot, N)
    D, A, P = e.D, e.A, env.pos_dim
    start, wp, nw = W.job(P)
    r = env.follow(e, start, wp, nw, max_steps=T, trace=(N, T), seed=FOLLOW_SEED, path_stride=1)
    assert r["persistent"] is True
    f = trace_fields(r["trace"], D, A)
    live = np.any(r["trace"] != 0, axis=2)
    _actor_error(p, f, live, f"{robot} {width} follow")
    for t in range(T):
        pos2, vel2, rew, reached = goal_advance(f["pos"][t], f["vel"][t], f["goal"][t], f["act"][t], env.mix, P, env.dt,
                                                env.extent, extra_bonus=env.extra_bonus)
        lv = live[t]
        assert np.max(np.abs(f["reward"][t][lv] - rew[lv]), initial=0.0) <= 2e-6
        assert np.array_equal(f["reached"][t][lv], reached[lv])
        if t + 1 < T:
            nxt = lv & live[t + 1]
            assert np.allclose(f["pos"][t + 1][nxt, :P], pos2[nxt], atol=2e-6)
            assert np.allclose(f["vel"][t + 1][nxt, :P], vel2[nxt], atol=2e-6)
        assert np.allclose(r["path"][t + 1][lv], pos2[lv], atol=2e-6)
    _check_trace(r, f, start, wp, nw, env, T, N)
    assert np.any((r["reached"] == nw) & (nw > 0)) and np.any(r["reached"] < nw)      # some robot finishes and some does not
    assert r["steps"][W.NO_WAYPOINTS] == 0 and not live[:, W.NO_WAYPOINTS].any()
    # the run split into calls, sampled actions
    kw = dict(seed=9, deterministic=False, leg_steps=40)
    fresh = FollowState(start, wp, nw, False, P)
    one = env.follow(e, max_steps=T, resume=fresh, **kw)
    got, state = None, fresh
    for _ in range(3):
        got = env.follow(e, max_steps=T // 3, resume=state, **kw)
        assert got["persistent"] is True
        state = got["state"]
    assert one["persistent"] is True and state.step0 == T
    for k in ("arrival", "reached", "steps", "reward_sum", "final_distance", "status"):
        assert np.array_equal(one[k], got[k], equal_nan=True), k
    _same({"state": one["state"]}, {"state": state}, "three calls")
    assert np.any(one["status"] != one["status"][0]) and one["steps"][W.NO_WAYPOINTS] == 0
    det = env.follow(e, max_steps=T, resume=fresh, seed=9, leg_steps=40)
    assert not np.array_equal(det["reward_sum"], one["reward_sum"]), "sampled actions should enter"
    e.close()


def _replay_schedule(r, f, env, rel, start, wp, nw):
    """tests/test_eval_tile256_gpu.py::test_schedule_holds over the call's own trace and path, and the hold record
    (goal_rules.schedule_fold) bit for bit"""
    P = env.pos_dim
    k, alive = np.zeros(N, int), nw > 0
    arrival = np.full((N, K), -1)
    held, anchor = np.zeros((T, N), bool), np.zeros((T, N, P), np.float32)
    for t in range(T):
        live = np.any(r["trace"][t] != 0, axis=1)
        assert np.array_equal(live, alive), f"step {t}: the robots that step"
        hold = Schedule.holding(rel, nw, k, t) & alive
        goal = Schedule.goal(rel, start, wp, nw, k, t)
        assert np.array_equal(f["goal"][t][alive, :P], goal[alive].astype(np.float32)), f"step {t}: the goal in force"
        assert np.all(f["reward"][t][hold] == 0) and not np.any(f["reached"][t][hold])
        _, _, _, reached = goal_advance(f["pos"][t], f["vel"][t], f["goal"][t], f["act"][t], env.mix, P, env.dt, env.extent,
                                        extra_bonus=env.extra_bonus)
        go = alive & ~hold
        assert np.array_equal(f["reached"][t][go], reached[go])
        held[t], anchor[t] = hold, np.where(hold[:, None], goal, 0.0)
        for i in np.nonzero(go & f["reached"][t])[0]:
            arrival[i, k[i]] = t + 1
            k[i] += 1
        alive = k < nw
    want = schedule_fold(np.tile(SCHED_START, (N, 1)), anchor, r["path"][1:], held)
    assert np.array_equal(r["state"].sched, want, equal_nan=True), (r["state"].sched, want)
    assert np.array_equal(r["hold_steps"], held.sum(0)) and np.any(r["hold_steps"] > 0) and np.any(r["hold_steps"] == 0)
    assert np.array_equal(r["arrival"], arrival) and np.array_equal(r["reached"], k)
    assert np.array_equal(r["lateness"], Schedule.lateness(rel, arrival), equal_nan=True)
    assert r["steps"][W.NO_WAYPOINTS] == 0
    return held


@pytest.mark.parametrize("robot", ["car", "turtlebot3"])
def test_schedule_on_the_256_tile(robot, persistent_env):
    """ScheduledFollowTask on k_goal256_tile at 8 and 12 layer-1 k-steps"""
    persistent_env(None)
    e, p = _make(robot, 256)
    env = _env(robot, N)
    start, wp, nw = W.job(env.pos_dim)
    rel = W.release()
    r = env.follow(e, start, wp, nw, max_steps=T, seed=FOLLOW_SEED, path_stride=1, trace=(N, T), schedule=Schedule(rel))
    assert r["persistent"] is True
    f = trace_fields(r["trace"], e.D, e.A)
    _actor_error(p, f, np.any(r["trace"] != 0, axis=2), f"{robot} 256 scheduled follow")
    _replay_schedule(r, f, env, rel, start, wp, nw)
    e.close()


@pytest.mark.parametrize("robot", W.WALL_ROBOTS)
def test_follow_with_everything_observational(robot, persistent_env):
    """WallTask<TeamTask<framed hazards<ScheduledFollowTask>>> (tests/test_walls_gpu.py::test_composition[all]) at DP = 32, 48, 16
    and 64: the carried wall, team and hold records from the rules over the call's own path, bit for bit; everything else as in
    the call without walls"""
    persistent_env(None)
    e, p = _make(robot, 64)
    env = _env(robot, N)
    D, A, P, Wd = e.D, e.A, env.pos_dim, 9 + e.D + e.A + 4
    start, wp, nw = W.job(P)
    rel = W.release()
    sched = Schedule(rel)
    kw = dict(max_steps=T, seed=FOLLOW_SEED, path_stride=1, trace=(N, T), schedule=sched)
    base = env.follow(e, resume=FollowState(start, wp, nw, False, P, False, sched), **kw)   # hazards and teams change no motion
    stepped = np.any(base["trace"] != 0, axis=2)
    full = [i for i in range(N) if base["steps"][i] == T]
    kw.update(hazards=_hazards_on(base["path"], W.spread(full, 3), "shaped"), teams=Teams(4, _separation(base["path"], stepped), 2.0))
    plain = env.follow(e, resume=FollowState(start, wp, nw, True, P, True, sched), **kw)
    assert base["persistent"] is True and plain["persistent"] is True and np.array_equal(base["path"], plain["path"])
    pre, post, stepped = _segments(plain)
    rows = W.spread(full, 6)
    boxes = [_crossing_box(pre, post, stepped, rows[0], 10), _contact_box(post, stepped, rows[1], 4)] + W.FAR
    boxes += [_crossing_box(pre, post, stepped, rows[2], 2), _contact_box(post, stepped, rows[3], 12),
              _crossing_box(pre, post, stepped, rows[4], 30), _contact_box(post, stepped, rows[5], 26)]
    walls = Walls(np.array(boxes), radius=W.RADIUS_WALL, cost=1.5, indicator=False)
    r = env.follow(e, start, wp, nw, walls=walls, **kw)
    assert r["persistent"] is True
    _same_outputs(plain, r, "walls change nothing else")
    _same_state(plain["state"], r["state"], "walls change nothing else", skip=("wall",))
    f = trace_fields(r["trace"], D, A)
    live = np.any(r["trace"][:, :, :Wd] != 0, axis=2)
    assert np.array_equal(live, stepped)
    _actor_error(p, f, live, f"{robot} 64 follow, everything observational")
    # walls
    want = wall_fold(np.tile(WALL_START, (N, 1)), pre, post, stepped, walls)
    assert np.array_equal(r["state"].wall, want, equal_nan=True), (r["state"].wall, want)
    assert np.any(r["crossing_steps"] > 0) and np.any(r["contact_steps"] > 0)
    assert np.array_equal(want[W.NO_WAYPOINTS], WALL_START, equal_nan=True)
    # teams
    want = team_fold(np.tile(TEAM_START, (N, 1)), _standing(r["path"], stepped), stepped, kw["teams"])
    assert np.array_equal(r["state"].team, want, equal_nan=True), (r["state"].team, want)
    _conflicts(r)
    # the schedule
    _replay_schedule(r, f, env, rel, start, wp, nw)
    # the hazard frames
    cost, clear = r["trace"][:, :, Wd], r["trace"][:, :, Wd + 1]
    post2 = np.zeros((T, N, 2), np.float32)
    post2[:] = r["path"][1:, :, :2]
    cmp_, left = _teacher_by_step(cost, clear, post2, live, kw["hazards"])
    _recount(cost, live, r, N)
    assert cmp_ > 0 and left <= 0.001 * cmp_
    _charged(r)
    assert np.any((r["reached"] == nw) & (nw > 0)) and np.any(r["reached"] < nw)
    e.close()


@pytest.mark.parametrize("with_", ["alone", "static", "teams"])
@pytest.mark.parametrize("robot", W.WALL_ROBOTS)
def test_solid_walls(robot, with_, persistent_env):
    """SolidFollowTask alone, under static hazards and under teams (tests/test_walls_solid_gpu.py) at DP = 32, 48, 16 and 64; for
    drone the first solid run with P = 3: z passes through unblocked"""
    persistent_env(None)
    e, p = _make(robot, 64)
    env = _env(robot, N)
    D, A, P, Wd = e.D, e.A, env.pos_dim, 9 + e.D + e.A + 4
    start, wp, nw = W.job(P)
    base = env.follow(e, max_steps=T, seed=FOLLOW_SEED, path_stride=1, trace=(N, T), resume=FollowState(start, wp, nw, pos_dim=P))
    stepped0 = np.any(base["trace"] != 0, axis=2)
    boxes, rows = W.solid_scene(base["steps"], base["path"], stepped0)
    kw, extra = {}, 0
    if with_ == "static":
        others = [i for i in range(N) if base["steps"][i] == T and i not in rows]
        kw["hazards"], extra = _hazards_on(base["path"], W.spread(others, 3), "static"), 2
    if with_ == "teams":
        kw["teams"] = Teams(4, _separation(base["path"], stepped0), 2.0)
    walls = Walls(boxes, radius=W.RADIUS_SOLID, cost=1.5, indicator=False, solid=True)
    r = env.follow(e, start, wp, nw, max_steps=T, seed=FOLLOW_SEED, path_stride=1, trace=(N, T), walls=walls, **kw)
    assert base["persistent"] is True and r["persistent"] is True
    code, inside, stepped = _teacher(r, env, walls, extra)       # goal_propose32, wall_block, wall_block_velocity: bit for bit
    want = wall_blocked_fold(np.tile(BLOCKED_START, (N, 1)), code, inside, stepped)
    print(f"{robot} {with_}: blocked steps {want[:, 0].tolist()} of robots {rows}")
    assert np.array_equal(r["state"].blocked, want)
    for k, v in blocked_result(r["state"]).items():
        assert np.array_equal(r[k], v)
    pre, post, _ = _segments(r)
    assert np.array_equal(r["state"].wall, wall_fold(np.tile(WALL_START, (N, 1)), pre, post, stepped, walls), equal_nan=True)
    f = trace_fields(r["trace"], D, A)
    _actor_error(p, f, stepped, f"{robot} 64 solid walls, {with_}")
    never = want[:, 0] == 0
    assert np.sum(~never) >= 3 and np.all(want[rows, 0] > 0) and np.any(never & (r["steps"] > 0))
    # a robot that is never blocked moves as it does without walls: every output is the base run's
    for k in base:
        if k not in ("state", "persistent", "trace", "path") and np.ndim(base[k]) >= 1 and len(base[k]) == N:
            assert np.array_equal(np.asarray(base[k])[never], np.asarray(r[k])[never], equal_nan=True), k
    assert np.array_equal(base["path"][:, never], r["path"][:, never])
    assert np.array_equal(base["trace"][:, never], r["trace"][:, never, :Wd])
    for fld in ("state", "robot", "arrival", "leg_used", "status"):
        assert np.array_equal(getattr(base["state"], fld)[never], getattr(r["state"], fld)[never], equal_nan=True), fld
    free = r["wall_inside_steps"] == 0
    assert np.all(r["crossing_steps"][free] == 0) and np.all(r["min_wall_clearance"][free & (r["steps"] > 0)] > -1e-6)
    for i in rows:                                            # (a car may end in the same corner of the arena either way)
        assert np.any(r["path"][:, i] != base["path"][:, i]), (i, "a blocked robot moves as if there were no wall")
    assert r["steps"][W.NO_WAYPOINTS] == 0 and np.any((r["reached"] == nw) & (nw > 0)) and np.any(r["reached"] < nw)
    if P == 3:                                                # z is no business of a wall: it moves in the blocked steps too
        for i in rows:
            t = int(np.flatnonzero(code[:, i])[0])
            assert r["path"][t + 1, i, 2] != r["path"][t, i, 2], (i, t)
    if with_ == "static":
        cost, clear = r["trace"][:, :, Wd], r["trace"][:, :, Wd + 1]
        post2 = np.zeros((T, N, 2), np.float32)
        post2[:] = r["path"][1:, :, :2]
        cmp_, left = _teacher_check(cost, clear, post2, stepped, lambda i: kw["hazards"].rows(i), 1.5, False)
        _recount(cost, stepped, r, N)
        assert cmp_ > 0 and left <= 0.001 * cmp_
        _charged(r)
    if with_ == "teams":                                      # the team check sees the resolved positions
        want = team_fold(np.tile(TEAM_START, (N, 1)), _standing(r["path"], stepped), stepped, kw["teams"])
        assert np.array_equal(r["state"].team, want, equal_nan=True)
        _conflicts(r)
    e.close()
