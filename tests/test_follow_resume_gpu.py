"""GPU: resumable waypoint following (mobrob_ppo_follow_waypoints_resume, FollowState, leg budgets, replanning).

Shapes: n = 21 robots (one full 16-robot tile of k_goal64_tile plus a partial one of 5), K = 4 waypoints, T = 48 steps, engines
built like tests/util._engine.  Two invariants carry the file: (I1) the first call of a run is the existing call, bit for bit;
(I2) a run split into calls ends with the carried arrays of one long call, bit for bit, on the same kernel path."""
import ctypes as C

import numpy as np
import pytest

from mobrob_amd.waypoints import FINISHED, GOING, STALLED, FollowState, follow_waypoints, follow_with_replanning
from tests.eval_model import goal_advance, trace_fields
from tests.test_follow_gpu import SQUARE, _paths, _square_starts, _tracker
from tests.util import EVAL_CASES as CASES, _engine, _env, _snapshot, persistent_env  # noqa: F401

pytestmark = pytest.mark.gpu

N, K, T = 21, 4, 48
ENGINES = [CASES[1], CASES[0], CASES[5], CASES[2]]          # point64, doggo64 (tile), doggo64 per-step, doggo256 (per-step, x3)
ENGINE_IDS = [c[0] for c in ENGINES]
SPLITS = [(1, 47), (16, 32), (47, 1), (16, 16, 16)]
FAR = 5.0                                                    # outside +-extent (3): never reached
SHARED = ("arrival", "reached", "steps", "reward_sum", "final_distance", "path", "trace", "persistent")
HAZARD_KEYS = ("cost_sum", "violation_steps", "first_violation", "min_clearance")


def _run_paths(n, K, P, seed):
    """Like test_follow_gpu._paths: even robots get waypoints a few cm apart (consecutive arrivals, they finish); odd robots a
    chain of waypoints 0.35 .. 0.7 apart from the start on (arrivals spread over the run, under whatever the policy does)."""
    start, wp = _paths(n, K, P, seed)
    rng = np.random.default_rng(1000 + seed)
    u = rng.standard_normal((n, K, P))
    u *= rng.uniform(0.35, 0.7, (n, K, 1)) / np.linalg.norm(u, axis=2, keepdims=True)
    chain = start[:, None, :] + np.cumsum(u, axis=1)
    wp = np.where((np.arange(n) % 2 == 1)[:, None, None], chain, wp).astype(np.float32)
    return start, wp


def _hazards(kind, n):
    from mobrob_amd.envs.goal_rules import Hazards
    rng = np.random.default_rng(4)
    if kind == "shared":                                     # one scene of 5 hazards: staged in LDS by the tile kernel
        return Hazards(rng.uniform(-1.5, 1.5, (5, 2)), 0.5, indicator=False)
    if kind == "scenes":                                     # a scene per robot: read from global memory
        return Hazards(rng.uniform(-1.5, 1.5, (n, 3, 2)), 0.5, indicator=False, scene=np.arange(n))
    return None


def _carried(r):
    s = r["state"]
    d = {"state": s.state, "robot": s.robot, "arrival": s.arrival, "leg_used": s.leg_used, "status": s.status}
    if s.hazard is not None:
        d["hazard"] = s.hazard
    return d


def _spread(r, bounds=(0, 16, 32, 48)):
    arr = r["arrival"][r["arrival"] > 0]
    return all(np.any((arr > lo) & (arr <= hi)) for lo, hi in zip(bounds[:-1], bounds[1:]))


def _one_call(e, env, guard, **kw):
    """The one-call run on the first path seed whose result passes `guard` (so that the comparison is not vacuous)."""
    P = env.pos_dim
    odd = np.arange(N) % 2 == 1
    for seed in range(40):
        start, wp = _run_paths(N, K, P, seed)
        # where the robots go when their goal is out of reach: the odd robots' waypoints are laid on that track, at steps spread
        # over the run, so that they arrive there (the goal direction is a small part of what this policy sees)
        probe = env.follow(e, start, np.full((N, 1, P), FAR, np.float32), max_steps=T, seed=9, path_stride=1,
                           deterministic=kw.get("deterministic", True))
        at = np.array([10, 22, 36, 46]) - np.random.default_rng(seed).integers(0, 6, K)
        wp[odd] = probe["path"][at][:, odd].transpose(1, 0, 2)
        fresh = FollowState(start, wp, None, kw.get("hazards") is not None, P)
        one = env.follow(e, max_steps=T, seed=9, resume=fresh, **kw)
        if guard(one):
            return fresh, one
    raise AssertionError("no path seed in 0 .. 39 gives a run that exercises the split")


def _chain(e, env, fresh, split, **kw):
    r, state = None, fresh
    for steps in split:
        r = env.follow(e, max_steps=steps, seed=9, resume=state, **kw)
        state = r["state"]
    return r


@pytest.mark.parametrize("case", ENGINES, ids=ENGINE_IDS)
def test_first_call_of_a_run_is_the_existing_call(case, persistent_env):
    name, robot, kw, pe, expect_persistent = case
    persistent_env(pe)
    e, _ = _engine(robot, kw)
    env = _env(robot, N)
    P = env.pos_dim
    start, wp = _run_paths(N, K, P, seed=2)
    nw = np.array([[K, K, 0, 2, K][i % 5] for i in range(N)], np.int32)
    for kind in (None, "shared", "scenes"):
        hz = _hazards(kind, N)
        args = dict(max_steps=T, seed=9, deterministic=False, path_stride=5, trace=(5, T), hazards=hz)
        old = env.follow(e, start, wp, nw, **args)
        new = env.follow(e, resume=FollowState(start, wp, nw, hz is not None, P), **args)
        assert old["persistent"] == expect_persistent and new["persistent"] == old["persistent"]
        for k in SHARED + (HAZARD_KEYS if hz is not None else ()):
            assert np.array_equal(old[k], new[k], equal_nan=True), (kind, k)
        assert "state" not in old and new["state"].step0 == T
        done = new["reached"] == nw
        assert np.array_equal(new["status"] == FINISHED, done & (nw > 0)) and np.all(new["status"][nw == 0] == 3)
        assert np.all(new["status"][~done] == GOING) and np.any(done & (nw > 0)) and np.any(~done)
    e.close()


@pytest.mark.parametrize("det", [True, False], ids=["det", "sampled"])
@pytest.mark.parametrize("case", ENGINES, ids=ENGINE_IDS)
def test_splitting_a_run_changes_nothing(case, det, persistent_env):
    name, robot, kw, pe, _ = case
    persistent_env(pe)
    e, _ = _engine(robot, kw)
    env = _env(robot, N)
    budget = lambda r: np.any(r["status"] == STALLED) and np.any(r["status"] == FINISHED)   # noqa: E731
    configs = [("plain", dict(), _spread, SPLITS), ("budget", dict(leg_steps=6), budget, SPLITS)]
    if not det:                                              # hazards once per engine: with sampled actions
        configs += [("shared scene", dict(hazards=_hazards("shared", N)), _spread, SPLITS),
                    ("scene per robot", dict(hazards=_hazards("scenes", N)), _spread, SPLITS[3:])]
    for label, cfg, guard, splits in configs:
        fresh, one = _one_call(e, env, guard, deterministic=det, **cfg)
        want = _carried(one)
        if "hazards" in cfg:
            assert np.any(one["cost_sum"] > 0)
        for split in splits:
            got = _chain(e, env, fresh, split, deterministic=det, **cfg)
            assert got["state"].step0 == T and got["persistent"] == one["persistent"]
            for k, v in _carried(got).items():
                assert np.array_equal(want[k], v, equal_nan=True), (label, split, k)
    e.close()


@pytest.mark.parametrize("case", [CASES[0], CASES[5]], ids=["doggo64", "doggo64_perstep"])
def test_budget_semantics_by_teacher_forcing(case, persistent_env):
    name, robot, kw, pe, _ = case
    persistent_env(pe)
    e, _ = _engine(robot, kw)
    env = _env(robot, N)
    D, A, P, R, B = e.D, e.A, env.pos_dim, 5, 6
    start, wp = _run_paths(N, K, P, seed=3)
    wp[1] = FAR                                              # robot 1 stalls on its first waypoint, whatever the policy does
    r = env.follow(e, max_steps=T, seed=9, trace=(R, T), leg_steps=B, resume=FollowState(start, wp, None, False, P))
    f = trace_fields(r["trace"], D, A)
    st = r["state"]
    k, leg, alive = np.zeros(R, int), np.zeros(R, int), np.ones(R, bool)
    stall_step = np.full(R, -1)
    for t in range(T):
        assert not np.any(r["trace"][t, ~alive]), f"step {t}: rows of idle robots stay zero"
        rows = np.nonzero(alive)[0]
        assert np.array_equal(f["goal"][t][rows, :P], wp[rows, k[rows]])
        assert np.array_equal(r["trace"][t, rows, -2], k[rows].astype(np.float32))
        _, _, rew, reached = goal_advance(f["pos"][t], f["vel"][t], f["goal"][t], f["act"][t], env.mix, P, env.dt, env.extent,
                                          extra_bonus=env.extra_bonus)
        assert np.array_equal(f["reached"][t][rows], reached[rows])
        for i in rows:
            if reached[i]:
                assert r["arrival"][i, k[i]] == t + 1
                k[i], leg[i] = k[i] + 1, 0
            else:
                leg[i] += 1
            if k[i] == K or leg[i] >= B:
                alive[i] = False
                stall_step[i] = t + 1 if k[i] < K else -1
    assert np.array_equal(st.leg_used[:R], leg) and np.array_equal(r["reached"][:R], k)
    want = np.where(k == K, FINISHED, np.where(leg >= B, STALLED, GOING))
    assert np.array_equal(r["status"][:R], want)
    stalled = np.nonzero(want == STALLED)[0]
    assert 1 in stalled and stall_step[1] == B and np.array_equal(r["steps"][stalled], stall_step[stalled])
    assert np.any(want == FINISHED)
    # ---- a stalled robot with new waypoints steps again: at the global step, from the carried pose and velocity ----
    new_wp = np.zeros((len(stalled), 2, P), np.float32)
    new_wp[:, 0] = st.positions[stalled] + 1.0
    new_wp[:, 1] = st.positions[stalled] + 1.5
    st.replan(stalled, new_wp)
    r2 = env.follow(e, max_steps=8, seed=9, trace=(R, 8), leg_steps=B, resume=st)
    f2 = trace_fields(r2["trace"], D, A)
    # the observation noise depends on (robot, global step) only: the same robots in the existing call, still going at step T
    ref = env.follow(e, start, np.full((N, 1, P), FAR, np.float32), max_steps=T + 1, seed=9, trace=(R, T + 1))
    noise = slice(3 * P, D)
    for i in stalled:
        assert np.array_equal(f2["pos"][0][i], st.state[i, :3]) and np.array_equal(f2["vel"][0][i], st.state[i, 3:])
        assert np.array_equal(f2["goal"][0][i, :P], new_wp[list(stalled).index(i), 0]) and r2["trace"][0, i, -2] == 0.0
        assert np.array_equal(f2["obs"][0][i][noise], trace_fields(ref["trace"], D, A)["obs"][T][i][noise])
        assert np.any(f2["obs"][0][i][noise] != trace_fields(ref["trace"], D, A)["obs"][0][i][noise])
        assert r2["steps"][i] > r["steps"][i] and r2["state"].leg_used[i] <= B
        assert np.all(r2["arrival"][i][r2["arrival"][i] > 0] > T)           # arrival steps are global
    others = [i for i in range(R) if i not in stalled and want[i] != GOING]
    assert not np.any(r2["trace"][:, others])
    e.close()


def test_replanning_end_to_end():
    n = 64
    env = _env("point", n)
    model = _tracker(env)
    start = _square_starts(n, seed=3)
    wp = np.full((1, 2), FAR)                                 # every robot is sent to a waypoint it cannot reach

    def planner(pos, status, reached):
        return {i: [[1.5, 1.5]] for i in np.nonzero(status == STALLED)[0]}

    r = follow_with_replanning(model, env, start, wp, planner, horizon=50, rounds=6, leg_steps=40, seed=4)
    assert r["persistent"] is True
    assert np.mean(r["status"] == FINISHED) >= 0.95, np.mean(r["status"] == FINISHED)
    assert np.all(r["round_status"][0] == STALLED) and np.all(r["steps"] > 40)
    r0 = follow_with_replanning(model, env, start, wp, lambda *a: {}, horizon=50, rounds=6, leg_steps=40, seed=4)
    assert not np.any(r0["status"] == FINISHED) and np.all(r0["status"] == STALLED) and np.all(r0["steps"] == 40)


def _call_resume(e, env, *, n=4, K=3, max_steps=20, step0=0, leg_steps=0, edit=None):
    """mobrob_ppo_follow_waypoints_resume straight through ctypes -> (rc, in/out arrays after, in/out arrays before)"""
    from mobrob_amd import _lib
    P = env.pos_dim
    g = e._goal_env_struct(P, env.mix, 0, False, env.dt, env.extent, 0.3, 5.0, 0.0, 0.1)
    sp = _lib.FollowSpec()
    sp.n_robots, sp.max_waypoints, sp.max_steps, sp.deterministic, sp.seed = n, K, max_steps, 1, 1
    a = {"state": np.zeros((n, 6), np.float32), "leg_used": np.zeros(n, np.int32), "status": np.full(n, 77, np.int32),
         "arrival": np.full((n, K), -1, np.int32), "robot": np.zeros((n, 4))}
    if edit:
        edit(a)
    before = {k: v.copy() for k, v in a.items()}
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    rs = _lib.FollowResume()
    rs.step0, rs.leg_steps = step0, leg_steps
    rs.state, rs.leg_used, rs.status = a["state"].ctypes.data_as(fp), a["leg_used"].ctypes.data_as(ip), a["status"].ctypes.data_as(ip)
    wp = np.full((n, K, P), 0.5, np.float32)
    rc = e.lib.mobrob_ppo_follow_waypoints_resume(e._h, C.byref(g), C.byref(sp), None, C.byref(rs), wp.ctypes.data_as(fp), None,
                                                   a["arrival"].ctypes.data_as(ip), a["robot"].ctypes.data_as(C.POINTER(C.c_double)),
                                                   None, None, None)
    return rc, a, before


@pytest.mark.parametrize("case", [CASES[0], CASES[2]], ids=["fused64", "x3_256"])
def test_invalid_runs_are_refused_untouched(case, persistent_env):
    from mobrob_amd import _lib
    name, robot, kw, pe, _ = case
    persistent_env(pe)
    e, _ = _engine(robot, kw)
    env = _env(robot, 4)

    def put(key, idx, v):
        return lambda a: a[key].__setitem__(idx, v)
    bad = [dict(step0=-1), dict(step0=2 ** 31 - 20, max_steps=20), dict(leg_steps=-1),
           dict(edit=put("state", (2, 1), np.nan)), dict(edit=put("state", (0, 4), np.inf)),
           dict(edit=put("leg_used", 1, 1)), dict(leg_steps=5, edit=put("leg_used", 1, 6)), dict(leg_steps=5, edit=put("leg_used", 3, -1)),
           dict(edit=put("robot", (1, 2), 4.0)), dict(edit=put("robot", (1, 2), -1.0)), dict(edit=put("robot", (3, 0), np.nan)),
           dict(edit=put("robot", (0, 0), -np.inf)),
           dict(edit=put("robot", (1, 2), 1.5)), dict(edit=put("robot", (2, 1), 0.5))]   # counts that are not whole numbers
    for b in bad:
        rc, after, before = _call_resume(e, env, **b)
        assert rc == _lib.ERR_INVALID, b
        for k in before:
            assert np.array_equal(after[k], before[k], equal_nan=True), (b, k)
    rc, after, _ = _call_resume(e, env, step0=2 ** 31 - 21, max_steps=20, leg_steps=5, edit=put("leg_used", 1, 5))
    assert rc in (0, 1) and np.all(after["status"] != 77) and after["status"][1] == STALLED and after["robot"][1, 1] == 0
    e.close()


@pytest.mark.parametrize("case", [CASES[0], CASES[2]], ids=["fused64", "x3_256"])
def test_a_resumed_run_does_not_interfere_with_training(case, persistent_env):
    from mobrob_amd.envs.vec_env import DeviceGoalVecEnv
    name, robot, kw, pe, _ = case
    persistent_env(pe)
    env_a = DeviceGoalVecEnv.for_robot(robot, 16, time_limit=40, seed=5)
    env_b = DeviceGoalVecEnv.for_robot(robot, 16, time_limit=40, seed=5)
    ea, _ = _engine(robot, kw, seed=7)
    eb, _ = _engine(robot, kw, seed=7)
    start, wp = _run_paths(33, K, env_b.pos_dim, seed=8)
    state = FollowState(start, wp, None, True, env_b.pos_dim)
    hz = _hazards("shared", 33)
    for it in range(2):
        env_a.collect(ea)
        env_b.collect(eb)
        state = env_b.follow(eb, max_steps=20, seed=3, deterministic=False, leg_steps=9, hazards=hz, resume=state,
                             path_stride=3, trace=(4, 10))["state"]
        sa, sb = _snapshot(ea, stats=False), _snapshot(eb, stats=False)
        for k in sa:
            assert np.array_equal(sa[k], sb[k]), f"iteration {it}: {k} differs after collect"
        ea.train()
        eb.train()
        assert np.array_equal(ea.get_flat_params(), eb.get_flat_params())
    assert state.step0 == 40
    ea.close()
    eb.close()


def test_host_and_device_agree_with_a_budget():
    """The rule and thresholds of test_follow_gpu.test_host_and_device_agree, on arrival and status: the square, then a fifth
    waypoint no robot can reach, a budget of 70 steps per waypoint."""
    n = 64
    env = _env("point", n)
    model = _tracker(env)
    start = _square_starts(n, seed=7)
    wp = np.concatenate([SQUARE, [[FAR, FAR]]]).astype(np.float32)
    dev = follow_waypoints(model, env, start, wp, max_steps=400, path_stride=1, seed=2, leg_steps=70)
    host = follow_waypoints(model, "point", start, wp, max_steps=400, path_stride=1, seed=2, leg_steps=70)
    assert host["persistent"] is None and dev["persistent"] is True
    assert np.mean(host["reached"] == dev["reached"]) >= 0.95
    assert np.mean(host["status"] == dev["status"]) >= 0.95
    assert np.mean(dev["status"] == STALLED) >= 0.95            # the budget ended the run, not the step cap
    both = (host["arrival"] > 0) & (dev["arrival"] > 0)
    assert both.sum() >= 0.9 * 4 * n
    diff = np.abs(host["arrival"][both] - dev["arrival"][both])
    assert np.mean(diff <= 1) >= 0.99, np.bincount(diff)
    same = both & (host["arrival"] == dev["arrival"])
    for i, k in zip(*np.nonzero(same)):
        t = dev["arrival"][i, k]
        assert np.max(np.abs(dev["path"][t, i] - host["path"][t, i])) <= 1e-3, (i, k)
    agree = host["status"] == dev["status"]
    assert np.array_equal(host["state"].leg_used[agree & (dev["status"] == STALLED)], np.full(np.sum(agree & (dev["status"] == STALLED)), 70))
