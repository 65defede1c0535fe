"""GPU: moving hazards on the device (mobrob_ppo_evaluate_goal_env_hazard_frames / mobrob_ppo_follow_waypoints_hazard_frames, a
goal_rules.MovingHazards wherever PPOEngine / DeviceGoalVecEnv / mobrob_amd.waypoints take `hazards`), over EVAL_CASES so that the
tile kernel and the per-step path, 64-wide, 256-wide, elu and gSDE engines all run.

Shapes: N = 40 robots (two full 16-robot tiles of k_goal64_tile and one half tile), T = 40 steps, M = 5 hazards in a shared scene
(staged in LDS by the tile kernel) or M = 9 in S = 3 per-robot scenes with ragged counts (read from global memory); neither M is
a multiple of 4, the width of the partial sums.  Two time axes of F = 3 frames: HOLD, frame_steps = 7 (the last frame is held
from step 21 on), and LOOP, frame_steps = 4 (wraps three times).  The hazards circle around the robots' starts and the
midpoints of their first legs, so that some robots are charged on many steps and some on none.

Teacher forcing uses test_hazards_gpu's comparison and bound (TOL = 1.5e-5: 16 float32 ulps at the largest hazard distance),
with the rows of the frame in force at each step."""
import ctypes as C

import numpy as np
import pytest

from mobrob_amd.envs import goal_rules as rules
from mobrob_amd.envs.goal_rules import MovingHazards
from mobrob_amd.waypoints import FollowState, follow_waypoints
from tests.eval_model import trace_fields
from tests.test_hazards_gpu import CORE_KEYS_EVAL, CORE_KEYS_FOLLOW, HAZARD_KEYS, TOL, _eq, _recount, _teacher_check
from tests.util import EVAL_CASES as CASES, EVAL_IDS as IDS, _engine, _env, _go_to_goal_params, _snapshot, persistent_env  # noqa: F401

pytestmark = pytest.mark.gpu

N, K, T, F = 40, 3, 40, 3
HOLD, LOOP = dict(frame_steps=7, loop=False), dict(frame_steps=4, loop=True)
AXES = [("hold7", HOLD), ("loop4", LOOP)]
COUNTS = np.array([9, 5, 2], np.int32)     # per-robot scenes, ragged: 9 and 5 are no multiples of 4, 2 leaves two quarters empty


def _paths(P, seed=12):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.5, 1.5, (N, P)).astype(np.float32), rng.uniform(-2.0, 2.0, (N, K, P)).astype(np.float32)


def _centres(start, wp, rows, M):
    """[M, 2]: alternately the start of a robot and the midpoint of its first leg, over the robots `rows`"""
    P = start.shape[1]
    c = np.zeros((M, 2))
    for j in range(M):
        i = rows[(j // 2) % len(rows)]
        p = start[i] if j % 2 == 0 else 0.5 * (start[i] + wp[i, 0])
        c[j, :min(P, 2)] = p[:2]
    return c


def _moving(kind, start, wp, axis, indicator=False, cost=1.5, identical=False):
    """The test's MovingHazards: hazards circling (radius of travel 0.3, 2 rad per frame) around the robots' starts / first legs,
    sizes 0.3 .. 0.45.  identical: every frame is frame 0 (the restage must not change the answer)."""
    rng = np.random.default_rng(3)
    if kind == "shared":
        M, kw = 5, {}
        cen = _centres(start, wp, np.arange(N), M)
    else:
        M, scene = 9, (np.arange(N) % 3).astype(np.int32)
        cen = np.stack([_centres(start, wp, np.nonzero(scene == s)[0], M) for s in range(3)])
        kw = dict(counts=COUNTS, scene=scene)
    size = rng.uniform(0.3, 0.45, M)
    mv = MovingHazards.circling(cen, 0.3, size, F, 2.0, cost=cost, indicator=indicator, **axis, **kw)
    if identical:
        mv.table[:] = mv.table[:, :1]
    return mv


def _static(mv, f=0):
    """frame f of `mv` as a goal_rules.Hazards"""
    t = mv.table[:, f]
    return rules.Hazards(t[..., :2] if mv.scene is not None else t[0, :, :2], t[..., 2] if mv.scene is not None else t[0, :, 2],
                         cost=mv.cost, indicator=mv.indicator, counts=mv.counts, scene=mv.scene)


def _assert_charged(r):
    """not vacuous: some robot is charged, and some robot is not charged on every step"""
    assert np.any(r["violation_steps"] > 0) and np.any(r["violation_steps"] < r["steps"]), (r["violation_steps"], r["steps"])


def _same(a, b, why):
    assert set(a) == set(b), why
    for k in a:
        if k == "state":
            for f in ("state", "robot", "arrival", "leg_used", "status", "hazard", "step0"):
                assert np.array_equal(getattr(a[k], f), getattr(b[k], f), equal_nan=True), (why, k, f)
        else:
            assert _eq(a[k], b[k]), (why, k)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_frame_and_identical_frames_are_the_static_call(case, persistent_env):
    name, robot, kw, pe, expect_persistent = case
    persistent_env(pe)
    e, _ = _engine(robot, kw)
    env = _env(robot, N, tl=15)
    P = env.pos_dim
    start, wp = _paths(P)
    det = bool(kw.get("use_sde"))
    for kind in ("shared", "scenes"):
        four = _moving(kind, start, wp, dict(frame_steps=3, loop=False), identical=True)      # F = 3 here, one more below
        four.table = np.ascontiguousarray(np.concatenate([four.table, four.table[:, :1]], axis=1))   # F = 4 identical frames
        assert four.n_frames == 4
        st = _static(four)
        one = MovingHazards(four.table[:, :1, :, :2] if kind == "scenes" else four.table[0, :1, :, :2],
                            four.table[:, 0, :, 2] if kind == "scenes" else four.table[0, 0, :, 2], frame_steps=5, cost=four.cost,
                            indicator=False, counts=four.counts, scene=four.scene)
        assert np.array_equal(one.table[:, 0], st.table)
        fol = dict(max_steps=T, seed=3, path_stride=3, trace=(N, T), deterministic=det)
        want = env.follow(e, start, wp, hazards=st, **fol)
        assert want["persistent"] == expect_persistent
        _assert_charged(want)
        for label, mv in (("F=1", one), ("F=4 identical", four)):
            _same(want, env.follow(e, start, wp, hazards=mv, **fol), (kind, label, "follow"))
        ev = dict(n_robots=N, max_steps=T, episodes=2 * N, seed=5, trace=(N, T), deterministic=det)
        want = env.evaluate(e, hazards=st, **ev)
        for label, mv in (("F=1", one), ("F=4 identical", four)):
            _same(want, env.evaluate(e, hazards=mv, **ev), (kind, label, "evaluate"))
        want = env.follow(e, hazards=st, resume=FollowState(start, wp, None, True, P), leg_steps=9, **fol)
        for label, mv in (("F=1", one), ("F=4 identical", four)):
            _same(want, env.follow(e, hazards=mv, resume=FollowState(start, wp, None, True, P), leg_steps=9, **fol), (kind, label, "run"))
    e.close()


def _teacher_by_step(cost, clear, post, live, mv, g0=0):
    """test_hazards_gpu._teacher_check row by row of the trace, each against the rows in force at its global step"""
    cmp_ = left = 0
    for t in range(live.shape[0]):
        if not live[t].any():
            continue
        only = np.zeros_like(live)
        only[t] = live[t]
        c, l_ = _teacher_check(cost, clear, post, only, lambda i, t=t: mv.rows(i, g0 + t), mv.cost, mv.indicator)
        cmp_, left = cmp_ + c, left + l_
    return cmp_, left


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_teacher_forcing(case, persistent_env):
    name, robot, kw, pe, expect_persistent = case
    persistent_env(pe)
    e, _ = _engine(robot, kw)
    env = _env(robot, N, tl=15)
    P, D, A = env.pos_dim, e.D, e.A
    W = 9 + D + A + 4
    start, wp = _paths(P)
    total = left = 0
    for kind in ("shared", "scenes"):
        for label, axis in AXES:
            # follow, shaped cost: post-step position = path record t + 1
            mv = _moving(kind, start, wp, axis, indicator=False)
            r = env.follow(e, start, wp, max_steps=T, seed=3, path_stride=1, trace=(N, T), hazards=mv)
            assert r["persistent"] == expect_persistent
            live = np.any(r["trace"][:, :, :W] != 0, axis=2)
            post = np.zeros((T, N, 2), np.float32)
            post[:, :, :min(P, 2)] = r["path"][1:, :, :2]
            cost, clear = r["trace"][:, :, W], r["trace"][:, :, W + 1]
            c, l_ = _teacher_by_step(cost, clear, post, live, mv)
            _recount(cost, live, r, N)                                    # hazard_out = the sums over the trace
            for i in range(N):
                if r["steps"][i] > 0:
                    assert r["min_clearance"][i] == np.min(clear[live[:, i], i]), i
            assert np.all(cost[~live] == 0) and np.all(clear[~live] == 0)
            _assert_charged(r)
            total, left = total + c, left + l_
            # evaluate, indicator: post-step position = the next trace row's state, where the step ended no episode; g = t
            mvi = _moving(kind, start, wp, axis, indicator=True, cost=1.0)
            ev = env.evaluate(e, n_robots=N, max_steps=T, seed=7, trace=(N, T), hazards=mvi)
            f = trace_fields(ev["trace"], D, A)
            live_e = np.any(ev["trace"][:, :, :W] != 0, axis=2)
            nxt = np.zeros_like(live_e)
            nxt[:-1] = live_e[:-1] & ~f["term"][:-1] & ~f["tr"][:-1]
            post_e = np.zeros((T, N, 2), np.float32)
            post_e[:-1] = f["pos"][1:, :, :2]
            if P == 1:
                post_e[..., 1] = 0
            cost_e, clear_e = ev["trace"][:, :, W], ev["trace"][:, :, W + 1]
            c, l_ = _teacher_by_step(cost_e, clear_e, post_e, nxt, mvi)
            _recount(cost_e, live_e, ev, N)
            assert np.any(ev["episodes"] > 0)                              # the clock ran through episode resets
            total, left = total + c, left + l_
    print(f"{name}: compared {total} rows, left out {left}")
    assert total > 0 and left <= 0.001 * total
    e.close()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_unchanged_core(case, persistent_env):
    name, robot, kw, pe, expect_persistent = case
    persistent_env(pe)
    e, _ = _engine(robot, kw)
    env = _env(robot, N, tl=15)
    start, wp = _paths(env.pos_dim, seed=4)
    W = 9 + e.D + e.A + 4
    det = bool(kw.get("use_sde"))
    mv = _moving("scenes", start, wp, LOOP)
    base = env.follow(e, start, wp, max_steps=T, seed=3, path_stride=1, trace=(N, T), deterministic=det)
    got = env.follow(e, start, wp, max_steps=T, seed=3, path_stride=1, trace=(N, T), deterministic=det, hazards=mv)
    assert base["persistent"] == expect_persistent
    for k in CORE_KEYS_FOLLOW:
        assert _eq(base[k], got[k]), k
    assert got["trace"].shape[2] == W + 2 and np.array_equal(base["trace"], got["trace"][:, :, :W])
    mv = _moving("shared", start, wp, HOLD)
    ev_b = env.evaluate(e, n_robots=N, max_steps=T, episodes=2 * N, seed=5, trace=(N, T), deterministic=det)
    ev_h = env.evaluate(e, n_robots=N, max_steps=T, episodes=2 * N, seed=5, trace=(N, T), deterministic=det, hazards=mv)
    for k in CORE_KEYS_EVAL:
        assert _eq(ev_b[k], ev_h[k]), k
    assert np.array_equal(ev_b["trace"], ev_h["trace"][:, :, :W])
    _assert_charged(got)
    e.close()


@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[2]], ids=["fused64", "generic_elu", "x3_256"])
def test_training_untouched(case, persistent_env):
    from mobrob_amd.envs.vec_env import DeviceGoalVecEnv
    name, robot, kw, pe, _ = case
    persistent_env(pe)
    env_a = DeviceGoalVecEnv.for_robot(robot, 16, time_limit=40, seed=5)
    env_b = DeviceGoalVecEnv.for_robot(robot, 16, time_limit=40, seed=5)
    ea, _ = _engine(robot, kw, seed=7)
    eb, _ = _engine(robot, kw, seed=7)
    start, wp = _paths(env_b.pos_dim, seed=8)
    mv = _moving("shared", start, wp, LOOP)
    state = FollowState(start, wp, None, True, env_b.pos_dim)
    for it in range(2):
        env_a.collect(ea)
        env_b.collect(eb)
        before = _snapshot(eb, stats=False)
        env_b.follow(eb, start, wp, max_steps=T, seed=it, hazards=mv, trace=(4, 10))
        state = env_b.follow(eb, max_steps=13, seed=3, hazards=mv, resume=state)["state"]
        env_b.evaluate(eb, n_robots=24, max_steps=T, seed=it, hazards=mv)
        sa, sb = _snapshot(ea, stats=False), _snapshot(eb, stats=False)
        for k in sa:
            assert np.array_equal(sa[k], sb[k]) and np.array_equal(before[k], sb[k]), f"iteration {it}: {k} differs"
        ea.train()
        eb.train()
        assert np.array_equal(ea.get_flat_params(), eb.get_flat_params())
    ea.close()
    eb.close()


def _late(mv):
    """`mv` with its last hazard in use far away in frames 0 and 1 and over the whole arena in frame 2: every robot is charged
    at the first check of frame 2, whatever it does"""
    for s in range(mv.n_scenes):
        j = int(mv.counts[s]) - 1
        mv.table[s, :2, j] = (9.0, 9.0, 0.1)
        mv.table[s, 2, j] = (0.0, 0.0, 10.0)
    return mv


def _chain(e, env, fresh, split, **kw):
    r, state = None, fresh
    for steps in split:
        r = env.follow(e, max_steps=steps, seed=9, resume=state, **kw)
        state = r["state"]
    return r


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_runs_split_into_calls(case, persistent_env):
    name, robot, kw, pe, expect_persistent = case
    persistent_env(pe)
    e, _ = _engine(robot, kw)
    env = _env(robot, N)
    P = env.pos_dim
    start, wp = _paths(P, seed=6)
    wp[1::2] = 5.0                                            # odd robots never arrive: they run all T steps
    det = bool(kw.get("use_sde"))
    for kind in ("shared", "scenes"):
        for label, axis in AXES:
            mv = _late(_moving(kind, start, wp, axis))
            fs = axis["frame_steps"]
            fresh = FollowState(start, wp, None, True, P)
            one = env.follow(e, max_steps=T, seed=9, resume=fresh, hazards=mv, deterministic=det)
            assert one["persistent"] == expect_persistent
            # first_violation is global: a robot clear of the circling hazards is first charged at the first check of frame 2
            assert np.any(one["first_violation"] == 2 * fs + 1) and np.all(one["first_violation"][1::2] <= 2 * fs + 1)
            assert np.all(one["first_violation"][1::2] > 0)
            for split in ((13, 27), (7, 7, 26)):
                got = _chain(e, env, fresh, split, hazards=mv, deterministic=det)
                assert got["persistent"] == one["persistent"]
                for f in ("state", "robot", "arrival", "leg_used", "status", "hazard", "step0"):
                    assert np.array_equal(getattr(one["state"], f), getattr(got["state"], f), equal_nan=True), (kind, label, split, f)
                for k in HAZARD_KEYS:
                    assert np.array_equal(one[k], got[k], equal_nan=True), (kind, label, split, k)
    # replan between calls keeps the hazard sums, and the robots left alone end where the one call ends
    mv = _late(_moving("shared", start, wp, HOLD))
    fresh = FollowState(start, wp, None, True, P)
    one = env.follow(e, max_steps=T, seed=9, resume=fresh, hazards=mv, deterministic=det)
    r1 = env.follow(e, max_steps=13, seed=9, resume=fresh, hazards=mv, deterministic=det)
    st = r1["state"]
    kept = st.hazard.copy()
    rows = np.array([1, 4, 17, 39])
    st.replan(rows, st.positions[rows][:, None, :] + 0.8)
    assert np.array_equal(st.hazard, kept, equal_nan=True)
    r2 = env.follow(e, max_steps=27, seed=9, resume=st, hazards=mv, deterministic=det)
    assert np.all(r2["cost_sum"] >= r1["cost_sum"]) and np.all(r2["violation_steps"] >= r1["violation_steps"])
    had = r1["first_violation"] > 0
    assert np.array_equal(r2["first_violation"][had], r1["first_violation"][had])
    assert np.all(r2["first_violation"][rows][~had[rows]] == 15)              # frame 2 from global step 14 on, replanned or not
    alone = np.setdiff1d(np.arange(N), rows)
    assert np.array_equal(r2["state"].hazard[alone], one["state"].hazard[alone], equal_nan=True)
    e.close()


def test_host_and_device_agree_on_moving_hazards():
    """test_hazards_gpu.test_host_and_device_first_violation's rule and margin with frames: same starts, waypoints and frames,
    deterministic actions, an actor that reads only the noise-free features.  Robot i is compared when every hazard pair of both
    trajectories, at the frame in force, lies farther from its boundary than the largest host / device position difference
    (plus TOL)."""
    from mobrob_amd.envs.vec_env import DeviceGoalVecEnv
    from mobrob_amd.rl_control.ppo import PPO
    env = DeviceGoalVecEnv.for_robot("point", N, time_limit=0, seed=0)
    model = PPO(env=env, n_steps=16, batch_size=64, seed=1)
    _go_to_goal_params(model.engine, env)
    sq = np.array([[1.0, 1.0], [1.0, -1.0], [-1.0, -1.0], [-1.0, 1.0]], np.float32)
    start = np.random.default_rng(7).uniform(-0.5, 0.5, (N, 2)).astype(np.float32)
    cen = np.array([[0.5, 0.5], [0.2, 0.2], [0.8, 0.9], [-0.2, 0.3], [0.4, -0.1]])
    compared = 0
    for label, axis in AXES:
        mv = MovingHazards.circling(cen, 0.3, [0.3, 0.25, 0.35, 0.2, 0.3], F, 2.0, cost=1.0, indicator=True, **axis)
        dev = follow_waypoints(model, env, start, sq, max_steps=T, path_stride=1, seed=2, hazards=mv)
        host = follow_waypoints(model, "point", start, sq, max_steps=T, path_stride=1, seed=2, hazards=mv)
        assert dev["persistent"] is True and host["persistent"] is None
        for i in range(N):
            S_ = int(max(dev["steps"][i], host["steps"][i]))
            pd, ph = dev["path"][1:S_ + 1, i].astype(np.float64), host["path"][1:S_ + 1, i].astype(np.float64)
            margin = float(np.max(np.abs(pd - ph))) + TOL
            rows = np.stack([mv.rows(i, g) for g in range(S_)])                  # [S_, M, 3]
            off = True
            for p in (pd, ph):
                d = np.hypot(p[:, None, 0] - rows[:, :, 0], p[:, None, 1] - rows[:, :, 1])
                off &= bool(np.all(np.abs(d - rows[:, :, 2]) > margin))
            if off and dev["steps"][i] == host["steps"][i]:
                compared += 1
                assert dev["first_violation"][i] == host["first_violation"][i], (label, i)
                assert dev["violation_steps"][i] == host["violation_steps"][i], (label, i)
        _assert_charged(dev)
    print(f"host vs device: {compared} of {2 * N} runs compared")
    assert compared >= N


def _call_frames(e, env, *, which="follow", n=4, S=1, Fr=2, M=2, frame_steps=3, loop=0, counts=None, scene=None, table=None,
                 run=False, hazard_out=True):
    """The *_hazard_frames entry points straight through ctypes with a hand-made mobrob_hazard_frames_t -> (rc, outputs)"""
    from mobrob_amd import _lib
    P, Kw, St = env.pos_dim, 2, 10
    g = e._goal_env_struct(P, env.mix, 0 if which == "follow" else 10, False, env.dt, env.extent, 0.3, 5.0, 0.0, 0.1)
    dp, fp, ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    h = _lib.HazardFramesC()
    t = np.full((max(S, 1), max(Fr, 1), max(M, 1), 3), 0.3, np.float32) if table is None else table
    keep = [t]
    h.n_scenes, h.max_hazards, h.hazards, h.cost, h.indicator = S, M, t.ctypes.data_as(fp), 1.0, 1
    h.n_frames, h.frame_steps, h.loop = Fr, frame_steps, loop
    for name_, arr in (("n_hazards", counts), ("scene", scene)):
        if arr is not None:
            keep.append(np.asarray(arr, np.int32))
            setattr(h, name_, keep[-1].ctypes.data_as(ip))
    robot, hzo = np.full((n, 4), 77.0), np.full((n, 4), 77.0)
    hz_ptr = hzo.ctypes.data_as(dp) if hazard_out else None
    if which == "evaluate":
        sp = _lib.EvalSpec()
        sp.n_robots, sp.max_steps, sp.episodes, sp.deterministic, sp.seed = n, St, 0, 1, 1
        rc = e.lib.mobrob_ppo_evaluate_goal_env_hazard_frames(e._h, C.byref(g), C.byref(sp), C.byref(h), None, robot.ctypes.data_as(dp),
                                                              None, hz_ptr, None, None)
        return rc, (robot, hzo)
    sp = _lib.FollowSpec()
    sp.n_robots, sp.max_waypoints, sp.max_steps, sp.deterministic, sp.seed = n, Kw, St, 1, 1
    start, wp = np.zeros((n, P), np.float32), np.ones((n, Kw, P), np.float32)
    arrival = np.full((n, Kw), 77, np.int32)
    rs = None
    if run:                                                   # the first call of a run: the values FollowState starts from
        rs = _lib.FollowResume()
        state, leg, status = np.zeros((n, 6), np.float32), np.zeros(n, np.int32), np.full(n, 77, np.int32)
        keep += [state, leg, status]
        rs.step0, rs.leg_steps, rs.state, rs.leg_used, rs.status = 0, 0, state.ctypes.data_as(fp), leg.ctypes.data_as(ip), status.ctypes.data_as(ip)
        robot[:], arrival[:] = 0.0, -1
        hzo[:] = (0.0, 0.0, -1.0, np.nan)
    rc = e.lib.mobrob_ppo_follow_waypoints_hazard_frames(e._h, C.byref(g), C.byref(sp), C.byref(h), None if rs is None else C.byref(rs),
                                                         start.ctypes.data_as(fp), wp.ctypes.data_as(fp), None, arrival.ctypes.data_as(ip),
                                                         robot.ctypes.data_as(dp), hz_ptr, None, None)
    return rc, (robot, hzo, arrival)


@pytest.mark.parametrize("case", [CASES[0], CASES[5], CASES[2]], ids=["fused64", "perstep64", "x3_256"])
def test_invalid_frames_are_refused(case, persistent_env):
    from mobrob_amd import _lib
    name, robot, kw, pe, _ = case
    persistent_env(pe)
    e, _ = _engine(robot, kw)
    env = _env(robot, 4)
    over = rules.HAZARD_FRAMES_MAX_BYTES // (1024 * 12) + 1                  # frames of 1024 hazards: one too many for the cap
    bad = {"frame_steps 0": dict(frame_steps=0), "frame_steps < 0": dict(frame_steps=-2), "F = 0": dict(Fr=0), "F < 0": dict(Fr=-1),
           "count > M": dict(counts=[3]), "over the cap": dict(Fr=over, M=1024, table=np.zeros((1, 1, 1024, 3), np.float32)),
           "S > 1 without scene": dict(S=2), "scene out of range": dict(S=2, scene=[0, 1, 2, 0]),
           "nan in the last frame": dict(table=np.array([[[[0, 0, 0.3]] * 2, [[0, 0, 0.3], [np.nan, 0, 0.3]]]], np.float32)),
           "no hazard_out": dict(hazard_out=False)}
    for which in ("follow", "evaluate"):
        for why, b in bad.items():
            rc, outs = _call_frames(e, env, which=which, **b)
            assert rc == _lib.ERR_INVALID, (which, why)
            assert all(np.all(o == 77) for o in outs), (which, why)
            if why == "over the cap":
                assert b"64 MiB" in e.lib.mobrob_ppo_last_error()
        rc, outs = _call_frames(e, env, which=which)                          # the engine is still usable
        assert rc in (0, 1) and np.all(outs[0][:, 1] == 10) and np.all(outs[1] != 77), which
        rc, outs = _call_frames(e, env, which=which, Fr=over - 1, M=1024, frame_steps=1,
                                table=np.full((1, over - 1, 1024, 3), 0.3, np.float32))   # exactly at the cap: taken
        assert rc in (0, 1), which
    rc, outs = _call_frames(e, env, run=True)
    assert rc in (0, 1) and np.all(outs[0][:, 1] == 10)
    rc, _ = _call_frames(e, env, run=True, hazard_out=False)                  # a run without hazard sums cannot take frames
    assert rc == _lib.ERR_INVALID
    # the Python surface: scene length != n, and a run started without hazards then continued with frames
    start, wp = np.zeros((4, env.pos_dim), np.float32), np.ones((4, 2, env.pos_dim), np.float32)
    short = MovingHazards(np.zeros((2, 2, 3, 2)), scene=[0, 1, 1])
    with pytest.raises(ValueError):
        env.follow(e, start, wp, max_steps=5, hazards=short)
    with pytest.raises(ValueError):
        env.evaluate(e, n_robots=4, max_steps=5, hazards=short)
    plain = env.follow(e, max_steps=5, resume=FollowState(start, wp, None, False, env.pos_dim))
    mv = MovingHazards(np.zeros((2, 3, 2)))
    with pytest.raises(ValueError):
        env.follow(e, max_steps=5, resume=plain["state"], hazards=mv)
    with pytest.raises(ValueError):
        follow_waypoints(e, env, max_steps=5, state=plain["state"], hazards=mv)
    with pytest.raises(TypeError):
        env.follow(e, start, wp, max_steps=5, hazards=mv.table)
    ok = env.follow(e, max_steps=5, resume=FollowState(start, wp, None, True, env.pos_dim), hazards=mv)
    assert np.all(ok["steps"] == 5) and ok["state"].step0 == 5
    e.close()
