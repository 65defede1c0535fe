"""GPU: the one-launch evaluation / waypoint-following kernel of fused 2x256 tanh engines (k_goal256_tile, csrc/kernels_eval256.h;
PPOEngine.set_eval_tile256).  It is off by default: every test here that wants it switches it on for its own engine.

Shapes: 8 robots (half a tile: rows beyond N), 16 (one tile), 20 and 33 (a full tile and a partial one / three tiles, the last
with one robot), 40 (early exit: three tiles), 4096 x 300 once for the statistical comparison with the per-step path.

The action bound of the teacher-forced traces is the one tests/test_eval_gpu.py holds the same engines to on the per-step path:
1e-5 * max(1, max|want|) against the float64 oracle on the traced observations.  Measured on the MI355X (the three evaluation
cases of test_teacher_forced_evaluation, printed by the test): 7.7e-7 doggo, 7.2e-7 point, 1.1e-6 drone
(profiles/r28/eval_tile256.txt)."""
import numpy as np
import pytest

from mobrob_amd.envs.goal_rules import Hazards, Schedule, Teams
from mobrob_amd.waypoints import FollowState
from oracle import ppo_oracle as O
from tests.eval_model import goal_advance, trace_fields
from tests.test_follow_gpu import _check_trace, _paths
from tests.util import EVAL_CASES as CASES, _engine, _env, _snapshot, persistent_env  # noqa: F401

pytestmark = pytest.mark.gpu

KW256 = dict(pi=(256, 256), vf=(256, 256))
CARRIED = ("state", "robot", "arrival", "leg_used", "status", "hazard", "team", "sched", "release", "home", "step0")


def _engine256(robot, on=True, **kw):
    e, p = _engine(robot, KW256, **kw)
    assert e.eval_tile256 is False
    if on:
        e.set_eval_tile256(True)
        assert e.eval_tile256 is True
    return e, p


def _same(a, b, why=""):
    """every output of two calls, bit for bit (a FollowState: its carried arrays)"""
    assert set(a) == set(b), why
    for k in a:
        if k == "state":
            for f in CARRIED:
                x, y = getattr(a[k], f, None), getattr(b[k], f, None)
                if not (x is None and y is None):
                    assert np.array_equal(x, y, equal_nan=True), (why, "state." + f)
        elif isinstance(a[k], np.ndarray) and a[k].dtype.kind == "f":
            assert np.array_equal(a[k], b[k], equal_nan=True), (why, k)
        else:
            assert np.array_equal(a[k], b[k]), (why, k)


@pytest.mark.parametrize("robot,R", [("doggo", 8), ("point", 33), ("drone", 16)])
def test_teacher_forced_evaluation(robot, R, persistent_env):
    """tests/test_eval_gpu.py::test_teacher_forced_trace on the tile: doggo (D = 58, A = 12; half a tile), point (D = 14: the
    observation tile is padding above 14; three tiles, the last with one robot), drone (A = 18: two head blocks, P = 3)."""
    persistent_env(None)
    e, p = _engine256(robot)
    env = _env(robot, R, tl=40)
    D, A, P = e.D, e.A, env.pos_dim
    S = 120
    r = env.evaluate(e, n_robots=R, max_steps=S, episodes=0, quota=np.full(R, 50, np.int32), trace=(R, S), seed=9)
    assert r["persistent"] is True
    f = trace_fields(r["trace"], D, A)
    mean, _ = O.policy_outputs(p, f["obs"].reshape(-1, D).astype(np.float32), activation="tanh")
    want = np.clip(mean, -1.0, 1.0).reshape(S, R, A)
    err, bound = float(np.max(np.abs(f["act"] - want))), 1e-5 * max(1.0, float(np.max(np.abs(want))))
    print(f"{robot}: tile action error {err:.3e} against the float64 oracle, bound {bound:.3e}")
    assert err <= bound
    for t in range(S):
        pos2, vel2, rew, reached = goal_advance(f["pos"][t], f["vel"][t], f["goal"][t], f["act"][t], env.mix, P, env.dt,
                                                env.extent, extra_bonus=env.extra_bonus)
        assert np.max(np.abs(f["reward"][t] - rew)) <= 2e-6
        assert np.array_equal(f["reached"][t], reached)
        if t + 1 == S:
            break
        done = f["term"][t] | f["tr"][t]
        cont = ~done
        assert np.allclose(f["pos"][t + 1][cont, :P], pos2[cont], atol=1e-6)
        assert np.allclose(f["vel"][t + 1][cont, :P], vel2[cont], atol=1e-6)
        assert np.array_equal(f["goal"][t + 1][cont], f["goal"][t][cont])
        rch = f["term"][t]   # lazy reset: pose kept, new goal in [-extent, extent]
        assert np.allclose(f["pos"][t + 1][rch, :P], pos2[rch], atol=1e-6)
        assert np.all(np.abs(f["goal"][t + 1][rch, :P]) <= env.extent)
        trc = f["tr"][t]     # truncation: fresh pose in [-extent/2, extent/2], zero velocity
        assert np.all(np.abs(f["pos"][t + 1][trc, :P]) <= env.extent / 2)
        assert np.all(f["vel"][t + 1][trc] == 0.0)
    assert f["tr"].any(), "the run should truncate some episodes (time_limit 40 < 120 steps)"
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
    e.close()


N, K, S = 20, 3, 90


def test_follow_teacher_forced(persistent_env):
    """tests/test_follow_gpu.py::test_teacher_forced_trace on the tile (FollowTask)"""
    persistent_env(None)
    e, p = _engine256("doggo")
    env = _env("doggo", N)
    D, A, P = e.D, e.A, env.pos_dim
    start, wp = _paths(N, K, P, seed=11, near_every=3)
    nw = np.full(N, K, np.int32)
    r = env.follow(e, start, wp, max_steps=S, trace=(N, S), seed=9, path_stride=1)
    assert r["persistent"] is True
    f = trace_fields(r["trace"], D, A)
    live = np.any(r["trace"] != 0, axis=2)
    mean, _ = O.policy_outputs(p, f["obs"][live].astype(np.float32), activation="tanh")
    want = np.clip(mean, -1.0, 1.0)
    assert np.max(np.abs(f["act"][live] - want)) <= 1e-5 * max(1.0, float(np.max(np.abs(want))))
    for t in range(S):
        pos2, vel2, rew, reached = goal_advance(f["pos"][t], f["vel"][t], f["goal"][t], f["act"][t], env.mix, P, env.dt,
                                                env.extent, extra_bonus=env.extra_bonus)
        lv = live[t]
        assert np.max(np.abs(f["reward"][t][lv] - rew[lv]), initial=0.0) <= 2e-6
        assert np.array_equal(f["reached"][t][lv], reached[lv])
        if t + 1 < S:
            nxt = lv & live[t + 1]
            assert np.allclose(f["pos"][t + 1][nxt, :P], pos2[nxt], atol=2e-6)
            assert np.allclose(f["vel"][t + 1][nxt, :P], vel2[nxt], atol=2e-6)
        assert np.allclose(r["path"][t + 1][lv], pos2[lv], atol=2e-6)
    _check_trace(r, f, start, wp, nw, env, S, N)
    assert np.any(r["reached"] == K) and np.any(r["reached"] < K)
    e.close()


def test_follow_run_split_into_calls(persistent_env):
    """ResumeFollowTask: the run as one call against three 30-step calls, sampled actions; the first call of a run is the plain
    call (FollowTask) bit for bit."""
    persistent_env(None)
    e, _ = _engine256("doggo")
    env = _env("doggo", N)
    P = env.pos_dim
    start, wp = _paths(N, K, P, seed=11, near_every=3)
    nw = np.array([[K, K, 0, 2, K][i % 5] for i in range(N)], np.int32)
    kw = dict(seed=9, deterministic=False, leg_steps=40)
    plain = env.follow(e, start, wp, nw, max_steps=S, seed=9, deterministic=False, path_stride=5, trace=(5, S))
    first = env.follow(e, resume=FollowState(start, wp, nw, False, P), max_steps=S, seed=9, deterministic=False, path_stride=5,
                       trace=(5, S))
    assert plain["persistent"] is True and first["persistent"] is True
    for k in ("arrival", "reached", "steps", "reward_sum", "final_distance", "path", "trace"):
        assert np.array_equal(plain[k], first[k], equal_nan=True), k
    fresh = FollowState(start, wp, nw, False, P)
    one = env.follow(e, max_steps=S, resume=fresh, **kw)
    r, state = None, fresh
    for _ in range(3):
        r = env.follow(e, max_steps=S // 3, resume=state, **kw)
        assert r["persistent"] is True
        state = r["state"]
    assert one["persistent"] is True and state.step0 == S
    assert np.any(one["reached"] > 0) and np.any(one["status"] != one["status"][0])
    for k in ("arrival", "reached", "steps", "reward_sum", "final_distance", "status"):
        assert np.array_equal(one[k], r[k], equal_nan=True), k
    _same({"state": one["state"]}, {"state": state}, "three calls")
    e.close()


def test_schedule_holds(persistent_env):
    """ScheduledFollowTask: release steps hold robots 2 and 5 at home; hold steps, arrivals and lateness equal the host rule's
    (goal_rules.Schedule) replayed over the traced steps."""
    persistent_env(None)
    e, _ = _engine256("doggo")
    env = _env("doggo", N)
    D, A, P = e.D, e.A, env.pos_dim
    start, wp = _paths(N, K, P, seed=11, near_every=3)
    nw = np.full(N, K, np.int32)
    rel = np.zeros((N, K), np.int32)
    rel[2, 0], rel[5, 0], rel[5, 1] = 12, 7, 30
    r = env.follow(e, start, wp, nw, max_steps=S, seed=3, path_stride=1, trace=(N, S), schedule=Schedule(rel))
    assert r["persistent"] is True
    f = trace_fields(r["trace"], D, A)
    k, alive = np.zeros(N, int), nw > 0
    holds, arrival = np.zeros(N, int), np.full((N, K), -1)
    for t in range(S):
        live = np.any(r["trace"][t] != 0, axis=1)
        assert np.array_equal(live, alive), f"step {t}: the robots that step"
        hold = Schedule.holding(rel, nw, k, t) & alive
        goal = Schedule.goal(rel, start, wp, nw, k, t)
        assert np.array_equal(f["goal"][t][alive, :P], goal[alive].astype(np.float32)), f"step {t}: the goal in force"
        assert np.all(f["reward"][t][hold] == 0) and not np.any(f["reached"][t][hold])
        _, _, _, reached = goal_advance(f["pos"][t], f["vel"][t], f["goal"][t], f["act"][t], env.mix, P, env.dt, env.extent,
                                        extra_bonus=env.extra_bonus)
        assert np.array_equal(f["reached"][t][alive & ~hold], reached[alive & ~hold])
        holds += hold
        for i in np.nonzero(alive & ~hold & reached)[0]:
            arrival[i, k[i]] = t + 1
            k[i] += 1
        alive = k < nw
    assert np.array_equal(r["hold_steps"], holds) and np.array_equal(np.nonzero(holds)[0], [2, 5])
    assert holds[2] == 12 and holds[5] >= 7
    assert np.array_equal(r["arrival"], arrival) and np.array_equal(r["reached"], k)
    assert np.array_equal(r["lateness"], Schedule.lateness(rel, arrival), equal_nan=True)
    assert np.all(arrival[2] > 12) or np.any(arrival[2] == -1)       # nothing arrives on a hold step
    e.close()


def test_determinism(persistent_env):
    persistent_env(None)
    e, _ = _engine256("doggo")
    env = _env("doggo", 33, tl=50)
    for det in (True, False):
        a, b = (env.evaluate(e, n_robots=33, max_steps=150, deterministic=det, seed=1, trace=(33, 20)) for _ in range(2))
        assert a["persistent"] is True and b["persistent"] is True
        for k in a:
            if isinstance(a[k], np.ndarray):
                assert a[k].tobytes() == b[k].tobytes(), (det, k)
    e.close()


def test_default_and_fallback(persistent_env, monkeypatch):
    persistent_env(None)
    monkeypatch.delenv("MOBROB_EVAL_TILE256", raising=False)
    e, _ = _engine256("doggo", on=False)
    env = _env("doggo", N, tl=40)
    P = env.pos_dim
    assert env.evaluate(e, n_robots=N, max_steps=20, seed=1)["persistent"] is False          # nothing set: as before
    monkeypatch.setenv("MOBROB_EVAL_TILE256", "1")                                            # an engine never told: the variable
    assert env.evaluate(e, n_robots=N, max_steps=20, seed=1)["persistent"] is True
    e.set_eval_tile256(False)                                                                 # told: the variable is not asked
    assert env.evaluate(e, n_robots=N, max_steps=20, seed=1)["persistent"] is False
    monkeypatch.delenv("MOBROB_EVAL_TILE256")
    # unserved tasks run the per-step path with the bits they have with the switch off
    start, wp = _paths(N, K, P, seed=11, near_every=3)
    nw = np.full(N, K, np.int32)
    hz = Hazards(np.random.default_rng(4).uniform(-1.5, 1.5, (5, 2)), 0.5, indicator=False)
    teams = Teams(4, 0.35, 2.0)
    outs = []
    for on in (False, True):
        e.set_eval_tile256(on)
        t = env.follow(e, resume=FollowState(start, wp, nw, False, P, True), max_steps=40, seed=9, teams=teams, path_stride=4)
        h = env.evaluate(e, n_robots=N, max_steps=40, seed=2, hazards=hz, trace=(N, 40))
        assert t["persistent"] is False and h["persistent"] is False
        outs.append((t, h))
    _same(outs[0][0], outs[1][0], "teams")
    _same(outs[0][1], outs[1][1], "hazards")
    # MOBROB_EVAL_PERSISTENT=0 forces the per-step path
    persistent_env("0")
    assert env.evaluate(e, n_robots=N, max_steps=20, seed=1)["persistent"] is False
    persistent_env(None)
    assert env.evaluate(e, n_robots=N, max_steps=20, seed=1)["persistent"] is True
    e.close()
    for robot, kw in (("doggo", dict(pi=(64, 64), vf=(64, 64))), ("point", dict(pi=(256, 256), vf=(256, 256), activation="elu"))):
        o, _ = _engine(robot, kw)
        with pytest.raises(ValueError, match="tile256"):
            o.set_eval_tile256(True)
        with pytest.raises(TypeError, match="tile256"):
            o.set_eval_tile256(1)
        assert o.eval_tile256 is False
        o.close()


def test_tile_and_per_step_paths_agree(persistent_env):
    """tests/test_eval_gpu.py::test_persistent_and_per_step_paths_agree on doggo 256: not bit-identical (f32 MFMA and the fast
    tanh against the per-step path's split-bf16 products), the two agree statistically."""
    persistent_env(None)
    e, _ = _engine256("doggo")
    env = _env("doggo", 4096, tl=100)
    a = env.evaluate(e, n_robots=4096, max_steps=300, episodes=0, quota=np.ones(4096, np.int32), seed=4)
    e.set_eval_tile256(False)
    b = env.evaluate(e, n_robots=4096, max_steps=300, episodes=0, quota=np.ones(4096, np.int32), seed=4)
    assert a["persistent"] and not b["persistent"]
    for k in ("reward_sum",):
        se = np.sqrt(a[k].var() / 4096 + b[k].var() / 4096)
        assert abs(a[k].mean() - b[k].mean()) <= 3 * se + 1e-9
    sa, sb = np.nan_to_num(a["episode_success"][:, 0]), np.nan_to_num(b["episode_success"][:, 0])
    assert abs(sa.mean() - sb.mean()) <= 3 * np.sqrt((sa.var() + sb.var()) / 4096) + 1e-9
    assert np.mean(a["episodes"] == b["episodes"]) >= 0.95
    e.close()


def test_tile_calls_do_not_interfere_with_training(persistent_env):
    """tests/test_eval_gpu.py::test_evaluation_does_not_interfere_with_training with tile calls in between"""
    persistent_env(None)
    robot = "doggo"
    env_a, env_b = _env(robot, 16, tl=40), _env(robot, 16, tl=40)
    ea, _ = _engine(robot, KW256, seed=7)
    eb, _ = _engine(robot, KW256, seed=7)
    eb.set_eval_tile256(True)
    P = env_b.pos_dim
    start, wp = _paths(17, K, P, seed=3)
    for it in range(3):
        env_a.collect(ea)
        env_b.collect(eb)
        assert env_b.evaluate(eb, n_robots=33, max_steps=60, seed=it)["persistent"] is True
        assert env_b.evaluate(eb, n_robots=5, episodes=7, seed=it + 10)["persistent"] is True
        sa, sb = _snapshot(ea), _snapshot(eb)
        for k in sa:
            if k == "stats_means":
                assert np.allclose(sa[k], sb[k], rtol=1e-12, atol=0, equal_nan=True), f"iteration {it}: {k}"
            else:
                assert np.array_equal(sa[k], sb[k]), f"iteration {it}: {k} differs after collect"
        recs = [sorted((r["r"], r["l"]) for r in x.episode_records(100)) for x in (ea, eb)]
        assert recs[0] == recs[1]
        ea.train()
        eb.train()
        assert env_b.follow(eb, start, wp, max_steps=30, seed=99)["persistent"] is True
        assert np.array_equal(ea.get_flat_params(), eb.get_flat_params())
    env_a.collect(ea)
    env_b.collect(eb)
    sa, sb = _snapshot(ea), _snapshot(eb)
    for k in ("obs", "actions", "rewards", "params", "m", "v"):
        assert np.array_equal(sa[k], sb[k]), k
    ea.close()
    eb.close()


def test_early_exit(persistent_env):
    """Every robot's waypoints lie a few cm apart, so all arrive within a few steps of a 400-step budget: the tiles leave the
    step loop through the published exit word.  Same bits as the call whose budget is the last arrival + 1."""
    persistent_env(None)
    e, _ = _engine256("doggo")
    n = 40
    env = _env("doggo", n)
    P = env.pos_dim
    start, wp = _paths(n, K, P, seed=5, near_every=1)
    nw = np.array([[K, 1, 0, 2][i % 4] for i in range(n)], np.int32)
    long = env.follow(e, start, wp, nw, max_steps=400, seed=9)
    assert long["persistent"] is True
    assert np.array_equal(long["reached"], nw), "every robot should finish"
    last = int(long["arrival"].max())
    assert last <= 20 and np.all(long["steps"] <= last)
    cut = env.follow(e, start, wp, nw, max_steps=last + 1, seed=9)
    for k in ("arrival", "reached", "steps", "reward_sum", "final_distance"):
        assert np.array_equal(long[k], cut[k], equal_nan=True), k
    e.close()
