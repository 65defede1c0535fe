"""GPU: calls WITH hazards on the one-launch kernel of fused 2x256 tanh engines (k_goal256_tile for the wide tasks,
csrc/kernels_eval256.h; PPOEngine.set_eval_tile256_wide).  Off by default, and it needs set_eval_tile256 as well.

Served: static and moving hazards on evaluate and follow, moving hazards on resumed runs, static hazards on scheduled runs.
Walls, solid walls, teams, static hazards on resumed runs and moving hazards on scheduled runs are NOT served (their tiles
spill vector registers or use scratch and are not built): such calls stay on the per-step path with the bits they
have there, which test_left_out_tasks_keep_their_path pins.

Shapes: 20 robots (two tiles, the second with 4), 3 waypoints, 90 steps, 5 hazards (a count that is no multiple of the four
quarters), a full trace and path_stride = 1; drone (A = 18: two head blocks, P = 3); 40 robots for the early exit.

Bounds: actions on the traced observations against the float64 oracle within 1e-5 * max(1, max|want|), the bound
tests/test_eval_tile256_gpu.py holds the non-wide tile to; the hazard columns with tests/test_hazards_gpu.py's checkers
(_teacher_check, _recount), as the 2x64 tile's tests do."""
import numpy as np
import pytest

from mobrob_amd.envs.goal_rules import Hazards, MovingHazards, Schedule, Teams, Walls
from mobrob_amd.waypoints import FollowState
from oracle import ppo_oracle as O
from tests.eval_model import goal_advance, trace_fields
from tests.test_eval_tile256_gpu import KW256, _same
from tests.test_follow_gpu import _check_trace, _paths
from tests.test_hazard_frames_gpu import _teacher_by_step
from tests.test_hazards_gpu import _recount, _teacher_check
from tests.util import _engine, _env, _snapshot, persistent_env  # noqa: F401

pytestmark = pytest.mark.gpu

N, K, S, M = 20, 3, 90, 5


def _engine_wide(robot="doggo", wide=True, **kw):
    e, p = _engine(robot, KW256, **kw)
    assert e.eval_tile256_wide is False
    e.set_eval_tile256(True)
    if wide:
        e.set_eval_tile256_wide(True)
        assert e.eval_tile256_wide is True
    return e, p


def _scene(base, m=M, radius=0.3):
    """m hazards ON the way of a base run (its path without hazards): robot i's position a third into its run, so the scene bites
    whatever the policy does.  Robots 0, 3, ... finish within a few steps (near waypoints): the others are used."""
    movers = [i for i in range(base["path"].shape[1]) if base["steps"][i] >= S // 2][:m]
    assert len(movers) == m
    xy = np.zeros((m, 2))
    P = min(base["path"].shape[2], 2)
    for j, i in enumerate(movers):
        xy[j, :P] = base["path"][S // 3, i, :P]
    return xy, np.linspace(0.2, radius, m)


def _moving(xy, size, **kw):
    """3 frames of 20 steps, held after the last: the scene drifts by 0.1 per frame"""
    loc = np.stack([xy + 0.1 * f for f in range(3)])
    return MovingHazards(loc, size, frame_steps=20, loop=False, **kw)


def _actions_within_bound(f, live, p):
    mean, _ = O.policy_outputs(p, f["obs"][live].astype(np.float32), activation="tanh")
    want = np.clip(mean, -1.0, 1.0)
    err, bound = float(np.max(np.abs(f["act"][live] - want))), 1e-5 * max(1.0, float(np.max(np.abs(want))))
    print(f"wide tile action error {err:.3e} against the float64 oracle, bound {bound:.3e}")
    assert err <= bound


def _follow_transitions(r, f, live, env, steps):
    """tests/test_eval_tile256_gpu.py::test_follow_teacher_forced's env check"""
    P = env.pos_dim
    for t in range(steps):
        pos2, vel2, rew, reached = goal_advance(f["pos"][t], f["vel"][t], f["goal"][t], f["act"][t], env.mix, P, env.dt,
                                                env.extent, extra_bonus=env.extra_bonus)
        lv = live[t]
        assert np.max(np.abs(f["reward"][t][lv] - rew[lv]), initial=0.0) <= 2e-6
        assert np.array_equal(f["reached"][t][lv], reached[lv])
        if t + 1 < steps:
            nxt = lv & live[t + 1]
            assert np.allclose(f["pos"][t + 1][nxt, :P], pos2[nxt], atol=2e-6)
            assert np.allclose(f["vel"][t + 1][nxt, :P], vel2[nxt], atol=2e-6)
        assert np.allclose(r["path"][t + 1][lv], pos2[lv], atol=2e-6)


def _hazard_columns(r, W, n, steps, rows_check):
    """the per-step cost / clearance columns against the rule at the pathed positions, and hazard_out recounted from them"""
    live = np.any(r["trace"][:, :, :W] != 0, axis=2)
    post = np.zeros((steps, n, 2), np.float32)
    post[:, :, :min(r["path"].shape[2], 2)] = r["path"][1:, :, :2]
    cost, clear = r["trace"][:, :, W], r["trace"][:, :, W + 1]
    cmp_, left = rows_check(cost, clear, post, live)
    _recount(cost, live, r, n)
    for i in range(n):
        if r["steps"][i] > 0:
            assert r["min_clearance"][i] == np.min(clear[live[:, i], i]), i
    assert np.all(cost[~live] == 0) and np.all(clear[~live] == 0)
    assert cmp_ > 0 and left <= 0.01 * cmp_ + 1
    assert np.any(r["cost_sum"] > 0) and np.any(r["violation_steps"] == 0), "the scene should charge some robots and spare some"
    return live


def _job(env, robot_n=N):
    start, wp = _paths(robot_n, K, env.pos_dim, seed=11, near_every=3)
    return start, wp, np.full(robot_n, K, np.int32)


def test_switch_semantics(persistent_env, monkeypatch):
    """The test that fails without the feature: a hazards call reports `persistent` True only with both switches in force."""
    persistent_env(None)
    monkeypatch.delenv("MOBROB_EVAL_TILE256", raising=False)
    monkeypatch.delenv("MOBROB_EVAL_TILE256_WIDE", raising=False)
    e, _ = _engine_wide(wide=False)
    env = _env("doggo", N, tl=40)
    start, wp, nw = _job(env)
    hz = Hazards(np.random.default_rng(4).uniform(-1.5, 1.5, (M, 2)), 0.5, indicator=False)
    mv = _moving(np.random.default_rng(4).uniform(-1.5, 1.5, (M, 2)), 0.5, indicator=False)

    def calls():
        return [env.evaluate(e, n_robots=N, max_steps=20, seed=2, hazards=hz)["persistent"],
                env.follow(e, start, wp, nw, max_steps=20, seed=2, hazards=hz)["persistent"],
                env.follow(e, resume=FollowState(start, wp, nw, True, env.pos_dim), max_steps=20, seed=2, hazards=mv)["persistent"]]
    assert calls() == [False] * 3                         # tile256 on, the wide switch never told
    monkeypatch.setenv("MOBROB_EVAL_TILE256_WIDE", "1")   # an engine never told: the variable
    assert calls() == [True] * 3
    e.set_eval_tile256_wide(False)                        # told: the variable is not asked
    assert calls() == [False] * 3
    monkeypatch.delenv("MOBROB_EVAL_TILE256_WIDE")
    e.set_eval_tile256_wide(True)
    assert calls() == [True] * 3 and e.eval_tile256_wide is True
    e.set_eval_tile256(False)                             # the wide switch alone is not enough
    assert calls() == [False] * 3
    e.set_eval_tile256(True)
    persistent_env("0")                                   # MOBROB_EVAL_PERSISTENT=0 forces the per-step path
    assert calls() == [False] * 3
    persistent_env(None)
    assert calls() == [True] * 3
    assert env.evaluate(e, n_robots=N, max_steps=20, seed=1)["persistent"] is True    # the non-wide tile as before
    e.close()
    for robot, kw in (("doggo", dict(pi=(64, 64), vf=(64, 64))), ("point", dict(pi=(256, 256), vf=(256, 256), activation="elu"))):
        o, _ = _engine(robot, kw)
        with pytest.raises(ValueError, match="tile256"):
            o.set_eval_tile256_wide(True)
        with pytest.raises(TypeError, match="tile256_wide"):
            o.set_eval_tile256_wide(1)
        assert o.eval_tile256_wide is False
        o.close()


@pytest.mark.parametrize("robot,n", [("doggo", N), ("drone", N)])
def test_teacher_forced_hazards_on_follow(robot, n, persistent_env):
    """HazardTask<FollowTask>; drone: A = 18 (two head blocks), P = 3"""
    persistent_env(None)
    e, p = _engine_wide(robot)
    env = _env(robot, n)
    D, A = e.D, e.A
    W = 9 + D + A + 4
    start, wp, nw = _job(env, n)
    base = env.follow(e, start, wp, nw, max_steps=S, seed=9, path_stride=1)
    xy, size = _scene(base)
    hz = Hazards(xy, size, cost=1.5, indicator=False)
    r = env.follow(e, start, wp, nw, max_steps=S, seed=9, path_stride=1, trace=(n, S), hazards=hz)
    assert r["persistent"] is True and r["trace"].shape[2] == W + 2
    f = trace_fields(r["trace"][:, :, :W], D, A)
    live = _hazard_columns(r, W, n, S, lambda c, cl, post, lv: _teacher_check(c, cl, post, lv, lambda i: hz.rows(i), 1.5, False))
    _actions_within_bound(f, live, p)
    _follow_transitions(r, f, live, env, S)
    _check_trace({**r, "trace": r["trace"][:, :, :W]}, f, start, wp, nw, env, S, n)
    assert np.any(r["reached"] == K) and np.any(r["reached"] < K)
    e.close()


def test_teacher_forced_hazards_on_evaluate(persistent_env):
    """HazardTask<EvalTask>, indicator cost, episodes ending inside the run: post-step position = the next row's state where the
    step ended no episode (tests/test_hazards_gpu.py::test_teacher_forcing)"""
    persistent_env(None)
    e, p = _engine_wide()
    env = _env("doggo", N, tl=40)
    D, A = e.D, e.A
    W = 9 + D + A + 4
    base = env.evaluate(e, n_robots=N, max_steps=S, seed=7, trace=(N, S))
    fb = trace_fields(base["trace"], D, A)
    xy = fb["pos"][S // 3, 1:1 + M, :2].astype(np.float64)
    hz = Hazards(xy, np.linspace(0.2, 0.3, M), cost=1.0, indicator=True)
    ev = env.evaluate(e, n_robots=N, max_steps=S, seed=7, trace=(N, S), hazards=hz, quota=np.full(N, 8, np.int32), episodes=0)
    assert ev["persistent"] is True
    f = trace_fields(ev["trace"][:, :, :W], D, A)
    live = np.any(ev["trace"][:, :, :W] != 0, axis=2)
    nxt = np.zeros_like(live)
    nxt[:-1] = live[:-1] & ~f["term"][:-1] & ~f["tr"][:-1]
    post = np.zeros((S, N, 2), np.float32)
    post[:-1] = f["pos"][1:, :, :2]
    cost, clear = ev["trace"][:, :, W], ev["trace"][:, :, W + 1]
    cmp_, left = _teacher_check(cost, clear, post, nxt, lambda i: hz.rows(i), 1.0, True)
    _recount(cost, live, ev, N)
    assert cmp_ > 0 and left <= 0.01 * cmp_ + 1
    assert np.any(ev["violation_steps"] > 0) and np.any(ev["episodes"] > 0)
    _actions_within_bound(f, live, p)
    e.close()


@pytest.mark.parametrize("kind", ["static_scheduled", "frames"])
def test_teacher_forced_hazards_on_runs(kind, persistent_env):
    """HazardTask<ScheduledFollowTask>: robots 2 and 5 held at home by release steps; FrameHazardTask<FollowTask>: 3 frames of 20
    steps (restaged at steps 20 and 40, held from then on)"""
    persistent_env(None)
    e, p = _engine_wide()
    env = _env("doggo", N)
    D, A, P = e.D, e.A, env.pos_dim
    W = 9 + D + A + 4
    start, wp, nw = _job(env)
    rel = np.zeros((N, K), np.int32)
    rel[2, 0], rel[5, 0] = 12, 7
    skw = dict(schedule=Schedule(rel)) if kind == "static_scheduled" else {}
    base = env.follow(e, start, wp, nw, max_steps=S, seed=9, path_stride=1, **skw)
    xy, size = _scene(base)
    skw = dict(schedule=Schedule(rel)) if kind == "static_scheduled" else {}
    if kind == "frames":
        mv = _moving(xy - 0.05, size, cost=1.5, indicator=False)
        check = lambda c, cl, post, lv: _teacher_by_step(c, cl, post, lv, mv)   # noqa: E731
    else:
        mv = Hazards(xy, size, cost=1.5, indicator=False)
        check = lambda c, cl, post, lv: _teacher_check(c, cl, post, lv, lambda i: mv.rows(i), 1.5, False)   # noqa: E731
    r = env.follow(e, start, wp, nw, max_steps=S, seed=9, path_stride=1, trace=(N, S), hazards=mv, **skw)
    assert r["persistent"] is True
    f = trace_fields(r["trace"][:, :, :W], D, A)
    live = _hazard_columns(r, W, N, S, check)
    _actions_within_bound(f, live, p)
    if kind == "static_scheduled":
        assert r["hold_steps"][2] == 12 and r["hold_steps"][5] >= 7
    else:
        # the frames differ where it matters: the static scene of frame 0 gives other costs
        st = env.follow(e, start, wp, nw, max_steps=S, seed=9, hazards=Hazards(xy - 0.05, size, cost=1.5, indicator=False))
        assert st["persistent"] is True and not np.array_equal(st["cost_sum"], r["cost_sum"])
    e.close()


@pytest.mark.parametrize("kind", ["frames"])
def test_split_run_equals_unsplit_run(kind, persistent_env):
    """FrameHazardTask<ResumeFollowTask> (HazardTask<ResumeFollowTask> is left out): 90 steps in one call = 3 calls of 30 through resume=, sampled actions"""
    persistent_env(None)
    e, _ = _engine_wide()
    env = _env("doggo", N)
    P = env.pos_dim
    start, wp, _ = _job(env)
    nw = np.array([[K, K, 0, 2, K][i % 5] for i in range(N)], np.int32)
    base = env.follow(e, start, wp, np.full(N, K, np.int32), max_steps=S, seed=9, path_stride=1)
    xy, size = _scene(base)
    hz = _moving(xy - 0.05, 0.6, cost=1.5, indicator=False)   # wide hazards: the sampled motion is not the base run's
    kw = dict(seed=9, deterministic=False, leg_steps=40, hazards=hz)
    fresh = FollowState(start, wp, nw, True, P)
    one = env.follow(e, max_steps=S, resume=fresh, **kw)
    r, state = None, fresh
    for _ in range(3):
        r = env.follow(e, max_steps=S // 3, resume=state, **kw)
        assert r["persistent"] is True
        state = r["state"]
    assert one["persistent"] is True and state.step0 == S and np.any(one["cost_sum"] > 0)
    for k in ("arrival", "reached", "steps", "reward_sum", "final_distance", "status", "cost_sum", "violation_steps",
              "first_violation", "min_clearance"):
        assert np.array_equal(one[k], r[k], equal_nan=True), k
    _same({"state": one["state"]}, {"state": state}, "three calls")
    e.close()


def test_determinism(persistent_env):
    persistent_env(None)
    e, _ = _engine_wide()
    env = _env("doggo", 33, tl=50)
    hz = Hazards(np.random.default_rng(4).uniform(-1.5, 1.5, (M, 2)), 0.5, indicator=False)
    for det in (True, False):
        a, b = (env.evaluate(e, n_robots=33, max_steps=150, deterministic=det, seed=1, trace=(33, 20), hazards=hz) for _ in range(2))
        assert a["persistent"] is True and b["persistent"] is True
        _same(a, b, f"deterministic={det}")
    e.close()


def test_early_exit(persistent_env):
    """tests/test_eval_tile256_gpu.py::test_early_exit with the wide phase between the last barrier and the exit word"""
    persistent_env(None)
    e, _ = _engine_wide()
    n = 40
    env = _env("doggo", n)
    start, wp = _paths(n, K, env.pos_dim, seed=5, near_every=1)
    nw = np.array([[K, 1, 0, 2][i % 4] for i in range(n)], np.int32)
    hz = Hazards(start[:M, :2].astype(np.float64) + 0.01, 0.2, cost=1.5, indicator=False)
    long = env.follow(e, start, wp, nw, max_steps=400, seed=9, hazards=hz)
    assert long["persistent"] is True
    assert np.array_equal(long["reached"], nw), "every robot should finish"
    last = int(long["arrival"].max())
    assert last <= 20 and np.all(long["steps"] <= last) and np.any(long["cost_sum"] > 0)
    cut = env.follow(e, start, wp, nw, max_steps=last + 1, seed=9, hazards=hz)
    for k in ("arrival", "reached", "steps", "reward_sum", "final_distance", "cost_sum", "violation_steps", "min_clearance"):
        assert np.array_equal(long[k], cut[k], equal_nan=True), k
    e.close()


def test_a_full_shared_scene_fits_and_per_robot_scenes_too(persistent_env):
    """1024 hazards (kHazardMax) in one shared scene: 12 KB + the xy block beside the tile's 150 416 bytes still fit the CU's LDS;
    the same hazards as per-robot scenes are read from global memory.  Both run the tile and give the same records."""
    persistent_env(None)
    e, _ = _engine_wide()
    env = _env("doggo", N)
    start, wp, nw = _job(env)
    xy = np.random.default_rng(8).uniform(-2.0, 2.0, (1024, 2))
    shared = env.follow(e, start, wp, nw, max_steps=30, seed=9, hazards=Hazards(xy, 0.05, cost=1.0, indicator=False))
    per = env.follow(e, start, wp, nw, max_steps=30, seed=9,
                     hazards=Hazards(np.stack([xy, xy]), 0.05, cost=1.0, indicator=False, scene=(np.arange(N) % 2).astype(np.int32)))
    assert shared["persistent"] is True and per["persistent"] is True
    for k in ("cost_sum", "violation_steps", "first_violation", "min_clearance", "arrival", "reward_sum"):
        assert np.array_equal(shared[k], per[k], equal_nan=True), k
    assert np.any(shared["cost_sum"] > 0)
    e.close()


def test_left_out_tasks_keep_their_path(persistent_env):
    """Walls, solid walls and teams are not served: with both switches on they report `persistent` False and give the bits they
    give with the switches off."""
    persistent_env(None)
    e, _ = _engine_wide(wide=False)
    env = _env("doggo", N)
    P = env.pos_dim
    start, wp, nw = _job(env)
    boxes = np.array([[0.0, 0.0, 0.3, 0.3], [1.0, -1.0, 0.2, 0.5], [-1.0, 0.5, 0.4, 0.1]])
    outs = []
    for on in (False, True):
        e.set_eval_tile256_wide(on)
        t = env.follow(e, resume=FollowState(start, wp, nw, False, P, True), max_steps=30, seed=9, teams=Teams(4, 0.35, 2.0))
        w = env.follow(e, start, wp, nw, max_steps=30, seed=9, walls=Walls(boxes, radius=0.1, cost=1.5, indicator=False))
        s = env.follow(e, start, wp, nw, max_steps=30, seed=9, walls=Walls(boxes, radius=0.1, cost=1.5, indicator=False, solid=True))
        assert t["persistent"] is False and w["persistent"] is False and s["persistent"] is False
        outs.append((t, w, s))
    for a, b, why in zip(outs[0], outs[1], ("teams", "walls", "solid")):
        _same(a, b, why)
    e.close()


def test_wide_tile_calls_do_not_interfere_with_training(persistent_env):
    """tests/test_eval_tile256_gpu.py::test_tile_calls_do_not_interfere_with_training with hazards calls in between"""
    persistent_env(None)
    robot = "doggo"
    env_a, env_b = _env(robot, 16, tl=40), _env(robot, 16, tl=40)
    ea, _ = _engine(robot, KW256, seed=7)
    eb, _ = _engine(robot, KW256, seed=7)
    eb.set_eval_tile256(True)
    eb.set_eval_tile256_wide(True)
    start, wp = _paths(17, K, env_b.pos_dim, seed=3)
    hz = Hazards(np.random.default_rng(4).uniform(-1.5, 1.5, (M, 2)), 0.5, indicator=False)
    for it in range(2):
        env_a.collect(ea)
        env_b.collect(eb)
        assert env_b.evaluate(eb, n_robots=33, max_steps=60, seed=it, hazards=hz)["persistent"] is True
        sa, sb = _snapshot(ea), _snapshot(eb)
        for k in sa:
            if k == "stats_means":
                assert np.allclose(sa[k], sb[k], rtol=1e-12, atol=0, equal_nan=True), f"iteration {it}: {k}"
            else:
                assert np.array_equal(sa[k], sb[k]), f"iteration {it}: {k} differs after collect"
        ea.train()
        eb.train()
        assert env_b.follow(eb, start, wp, max_steps=30, seed=99, hazards=hz)["persistent"] is True
        assert np.array_equal(ea.get_flat_params(), eb.get_flat_params())
    env_a.collect(ea)
    env_b.collect(eb)
    sa, sb = _snapshot(ea), _snapshot(eb)
    for k in ("obs", "actions", "rewards", "params", "m", "v"):
        assert np.array_equal(sa[k], sb[k]), k
    ea.close()
    eb.close()
