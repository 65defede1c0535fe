"""GPU: robot teams on the device (mobrob_ppo_follow_waypoints_teams; `teams=` on PPOEngine.follow_waypoints, DeviceGoalVecEnv.follow
and mobrob_amd.waypoints), over EVAL_CASES so that the tile kernel and the per-step path (k_team_step), 64-wide, 256-wide, elu and
gSDE engines all run, with the hazard tests' hand-built go-to-goal actor: motion is deterministic and conflicts certain.

Shapes (robots, team size): (20, 4) -- a last tile of one team and twelve empty lanes; (18, 2); (32, 16) and (32, 8) -- two
teams per tile, quarters with 4 and 2 members; team size 2 leaves two quarters empty, 4 gives one member each.  T = 48 steps.
In every team the members start on a circle of radius 0.8 around one point and head for the antipode and back, so all paths of
a team cross near its centre, twice; in every odd team member 0 has no waypoints and stands far away: it is never charged (and a
team of 2 with it has no conflict at all).  Teams lie on top of each other: they must not see each other.

Teacher forcing is exact: team_out is recomputed with goal_rules.team_fold from the traced live flags and the path's post-step
positions and must be equal bit for bit."""
import ctypes as C

import numpy as np
import pytest

from mobrob_amd.envs import goal_rules as rules
from mobrob_amd.envs.goal_rules import TEAM_START, MovingHazards, Teams, team_fold
from mobrob_amd.waypoints import FINISHED, FollowState, follow_waypoints
from tests.test_hazards_gpu import TOL, _eq, _go_to_goal
from tests.util import EVAL_CASES as CASES, EVAL_IDS as IDS, _engine, _env, _go_to_goal_params, _snapshot, persistent_env  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPES = [(20, 4), (18, 2), (32, 16), (32, 8)]
T, K, SEP = 48, 2, 0.35
TEAM_KEYS = ("team_cost_sum", "conflict_steps", "first_conflict", "min_team_clearance", "closest_partner")
CARRIED = ("state", "robot", "arrival", "leg_used", "status", "hazard", "team", "step0")


def _job(n, G, P, seed=0):
    """-> start [n][P], waypoints [n][K][P], counts [n] (see the module docstring)"""
    rng = np.random.default_rng(seed)
    start, wp, nw = np.zeros((n, P), np.float32), np.zeros((n, K, P), np.float32), np.full(n, K, np.int32)
    for i in range(n):
        k, m = divmod(i, G)
        c = 0.1 * np.array([np.cos(k), np.sin(k)])
        a = 2 * np.pi * m / max(G, 2) + 0.37 * k
        r = 0.8 + (0.05 * rng.random() if i % 2 else 0.0)
        u = np.array([np.cos(a), np.sin(a)])
        start[i, :2], wp[i, 0, :2], wp[i, 1, :2] = c + r * u, c - r * u, c + r * u
        if k % 2 == 1 and m == 0:
            start[i, :2], nw[i] = (2.3, -2.3), 0
    if P > 2:
        start[:, 2:] = wp[:, :, 2:] = 0.5
    return start, wp, nw


def _hazards(kind, start):
    if kind is None:
        return None
    xy = np.array([[0.0, 0.0], [0.4, 0.3], [-0.5, 0.2]])
    if kind == "static":
        return rules.Hazards(xy, [0.3, 0.2, 0.25], cost=1.5, indicator=False)
    return MovingHazards.circling(xy, 0.3, [0.3, 0.2, 0.25], 3, 2.0, cost=1.5, indicator=False, frame_steps=7, loop=True)


def _state(start, wp, nw, hz, P, teams=True):
    return FollowState(start, wp, nw, hz is not None, P, teams)


def _same_state(a, b, why, skip=()):
    for f in CARRIED:
        if f not in skip and not (getattr(a, f) is None and getattr(b, f) is None):
            assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), (why, f)


def _charged_and_free(r):
    """a condition on the inputs: a robot with conflict steps and a robot without"""
    assert np.any(r["conflict_steps"] > 0) and np.any(r["conflict_steps"] == 0), r["conflict_steps"]


def _setup(case, persistent_env, n):
    name, robot, kw, pe, expect_persistent = case
    persistent_env(pe)
    e, _ = _engine(robot, kw)
    env = _env(robot, n)
    _go_to_goal(e, env)
    return e, env, True, expect_persistent   # deterministic actions: the motion is the actor's


def test_the_setup_on_the_host_rule():
    """the jobs meet the charged-and-free condition on straight-line motion at the actor's speed (CPU only, the host rule)"""
    for n, G in SHAPES:
        start, wp, nw = _job(n, G, 2)
        t = np.arange(1, T + 1)[:, None, None] * 0.05
        d = wp[:, 0] - start
        L = np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-9)
        pos = start[None] + np.minimum(t, L[None]) * (d / L)[None]
        rec = team_fold(np.tile(TEAM_START, (n, 1)), pos, np.broadcast_to(nw > 0, (T, n)), Teams(G, SEP))
        assert np.any(rec[:, 1] > 0) and np.any(rec[:, 1] == 0), (n, G)


@pytest.mark.parametrize("shape", SHAPES, ids=[f"n{n}g{g}" for n, g in SHAPES])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_teacher_forcing(case, shape, persistent_env):
    n, G = shape
    e, env, det, expect_persistent = _setup(case, persistent_env, n)
    P = env.pos_dim
    W = 9 + e.D + e.A + 4
    start, wp, nw = _job(n, G, P)
    for indicator in (False, True):
        teams = Teams(G, SEP, 2.5, indicator)
        r = env.follow(e, start, wp, nw, max_steps=T, seed=3, path_stride=1, trace=(n, T), deterministic=det, teams=teams)
        assert r["persistent"] == expect_persistent and r["trace"].shape[2] == W
        live = np.any(r["trace"] != 0, axis=2)
        assert np.array_equal(live.sum(0), r["steps"])
        post = np.zeros((T, n, 2), np.float32)
        post[:, :, :min(P, 2)] = r["path"][1:, :, :2]
        want = team_fold(np.tile(TEAM_START, (n, 1)), post, live, teams)
        got = r["state"].team
        print(f"{case[0]} n={n} G={G} indicator={indicator}: conflict steps {got[:, 1].astype(int).tolist()}")
        for col, what in enumerate(("cost sum", "conflict steps", "first conflict", "min clearance", "partner")):
            assert np.array_equal(want[:, col], got[:, col], equal_nan=True), (what, want[:, col], got[:, col])
        _charged_and_free(r)
        assert np.all(np.isnan(got[nw == 0, 3])) and np.all(got[nw == 0, :2] == 0)
        part = r["closest_partner"]
        assert np.all((part < 0) | ((part // G == np.arange(n) // G) & (part != np.arange(n))))
    e.close()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_unchanged_core(case, persistent_env):
    n, G = 20, 4
    e, env, det, expect_persistent = _setup(case, persistent_env, n)
    P = env.pos_dim
    start, wp, nw = _job(n, G, P)
    for kind in (None, "static", "moving"):
        hz = _hazards(kind, start)
        kw = dict(max_steps=T, seed=3, path_stride=1, trace=(n, T), deterministic=det, hazards=hz, leg_steps=30)
        base = env.follow(e, resume=_state(start, wp, nw, hz, P, False), **kw)
        for G_ in (G, 1):
            got = env.follow(e, resume=_state(start, wp, nw, hz, P), teams=Teams(G_, SEP), **kw)
            assert base["persistent"] == expect_persistent == got["persistent"]
            assert set(got) == set(base) | set(TEAM_KEYS)
            for k in base:
                if k == "state":
                    _same_state(base[k], got[k], (kind, G_), skip=("team",))
                else:
                    assert _eq(base[k], got[k]), (kind, G_, k)
            if G_ == 1:                                            # the empty record: +inf once a step was run
                ran = got["steps"] > 0
                assert np.array_equal(got["state"].team[ran], np.tile([0.0, 0.0, -1.0, np.inf, -1.0], (ran.sum(), 1)))
                assert np.array_equal(got["state"].team[~ran], np.tile(TEAM_START, ((~ran).sum(), 1)), equal_nan=True)
            else:
                _charged_and_free(got)
        if hz is not None:
            assert np.any(base["violation_steps"] > 0)
    e.close()


def _chain(e, env, fresh, split, **kw):
    r, state = None, fresh
    for steps in split:
        r = env.follow(e, max_steps=steps, resume=state, **kw)
        state = r["state"]
    return r


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_runs_split_into_calls(case, persistent_env):
    n, G = 18, 2
    e, env, det, expect_persistent = _setup(case, persistent_env, n)
    P = env.pos_dim
    start, wp, nw = _job(n, G, P)
    # team 0: robot 0 finishes within the first call, robot 1 passes it, 0.05 off, in the second
    start[0, :2], wp[0, 0, :2], nw[0] = (-0.4, 0.0), (0.0, 0.0), 1
    start[1, :2], wp[1, 0, :2], nw[1] = (-2.2, 0.05), (1.6, 0.05), 1
    teams = Teams(G, SEP, 2.0)
    for kind in (None, "moving"):
        hz = _hazards(kind, start)
        kw = dict(seed=9, deterministic=det, hazards=hz, teams=teams)
        fresh = _state(start, wp, nw, hz, P)
        one = env.follow(e, max_steps=60, resume=fresh, **kw)
        assert one["persistent"] == expect_persistent
        _charged_and_free(one)
        for split in ((25, 35), (1, 59)):
            got = _chain(e, env, fresh, split, **kw)
            _same_state(one["state"], got["state"], (kind, split))
            for k in TEAM_KEYS:
                assert np.array_equal(one[k], got[k], equal_nan=True), (kind, split, k)
        first = env.follow(e, max_steps=25, resume=fresh, **kw)
        assert first["status"][0] == FINISHED and first["conflict_steps"][1] == 0        # parked before its mate comes by
        assert one["first_conflict"][1] > 25 and one["team_cost_sum"][1] > 0 and one["closest_partner"][1] == 0
        assert one["conflict_steps"][0] == 0                                              # the parked robot accounts nothing
    # a replan between the calls keeps the team sums; the robots left alone end where the one call ends
    st = first["state"]
    kept = st.team.copy()
    rows = np.array([3, 8])
    st.replan(rows, st.positions[rows][:, None, :] + 0.5)
    assert np.array_equal(st.team, kept, equal_nan=True)
    r2 = env.follow(e, max_steps=35, resume=st, **kw)
    assert np.all(r2["team_cost_sum"] >= first["team_cost_sum"]) and np.all(r2["conflict_steps"] >= first["conflict_steps"])
    had = first["first_conflict"] > 0
    assert np.array_equal(r2["first_conflict"][had], first["first_conflict"][had])
    alone = np.setdiff1d(np.arange(n), [2, 3, 8, 9])                                      # the teams without a replanned robot
    assert np.array_equal(r2["state"].team[alone], one["state"].team[alone], equal_nan=True)
    e.close()


def test_host_and_device_agree():
    """One team of four on a point robot, same starts: the host loop (float64 dynamics) against the device (float32), with the
    actor that reads only the noise-free features.  Robot i is compared when every mate distance of both trajectories lies
    farther from the separation, and its two smallest clearances lie farther from each other, than twice the largest host /
    device position difference plus TOL (test_hazards_gpu's margin rule, two moving ends); the sums within TOL."""
    from mobrob_amd.envs.vec_env import DeviceGoalVecEnv
    from mobrob_amd.rl_control.ppo import PPO
    n = 4
    env = DeviceGoalVecEnv.for_robot("point", n, time_limit=0, seed=0)
    model = PPO(env=env, n_steps=16, batch_size=64, seed=1)
    _go_to_goal_params(model.engine, env)
    start = np.array([[-0.9, 0.0], [0.8, 0.1], [0.05, -0.85], [2.0, 2.0]], np.float32)
    wp = np.array([[[0.9, 0.05]], [[-0.8, 0.0]], [[0.0, 0.9]], [[2.0, 2.0]]], np.float32)
    nw = np.array([1, 1, 1, 0])
    teams = Teams(4, 0.3, 1.0)
    dev = follow_waypoints(model, env, start, wp, nw, max_steps=T, path_stride=1, seed=2, teams=teams)
    host = follow_waypoints(model, "point", start, wp, nw, max_steps=T, path_stride=1, seed=2, teams=teams)
    assert dev["persistent"] is True and host["persistent"] is None
    pd, ph = dev["path"][1:].astype(np.float64), host["path"][1:].astype(np.float64)
    margin = 2 * float(np.max(np.abs(pd - ph))) + TOL
    compared = 0
    for i in range(n):
        ok = dev["steps"][i] == host["steps"][i]
        for p in (pd, ph):
            d = np.delete(np.hypot(*(p[:, i, None] - p).transpose(2, 0, 1)), i, axis=1)          # [T][3]
            s = np.sort(d, axis=1)
            ok &= bool(np.all(np.abs(d - teams.separation) > margin)) and bool(np.all(s[:, 1] - s[:, 0] > margin))
        if ok:
            compared += 1
            for k in ("conflict_steps", "first_conflict", "closest_partner"):
                assert dev[k][i] == host[k][i], (k, i)
        print(f"robot {i}: cost sum device {dev['team_cost_sum'][i]!r} host {host['team_cost_sum'][i]!r}")
        assert abs(dev["team_cost_sum"][i] - host["team_cost_sum"][i]) <= TOL, i
    print(f"host vs device: {compared} of {n} robots compared, margin {margin:.3g}")
    assert compared >= 2
    _charged_and_free(dev)


@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[2]], ids=["fused64", "generic_elu", "x3_256"])
def test_training_untouched(case, persistent_env):
    from mobrob_amd.envs.vec_env import DeviceGoalVecEnv
    name, robot, kw, pe, _ = case
    persistent_env(pe)
    env_a = DeviceGoalVecEnv.for_robot(robot, 16, time_limit=40, seed=5)
    env_b = DeviceGoalVecEnv.for_robot(robot, 16, time_limit=40, seed=5)
    ea, _ = _engine(robot, kw, seed=7)
    eb, _ = _engine(robot, kw, seed=7)
    start, wp, nw = _job(20, 4, env_b.pos_dim)
    teams = Teams(4, SEP)
    state = _state(start, wp, nw, None, env_b.pos_dim)
    for it in range(2):
        env_a.collect(ea)
        env_b.collect(eb)
        before = _snapshot(eb, stats=False)
        env_b.follow(eb, start, wp, nw, max_steps=T, seed=it, teams=teams, trace=(4, 10), hazards=_hazards("static", start))
        state = env_b.follow(eb, max_steps=13, seed=3, teams=teams, resume=state)["state"]
        sa, sb = _snapshot(ea, stats=False), _snapshot(eb, stats=False)
        for k in sa:
            assert np.array_equal(sa[k], sb[k]) and np.array_equal(before[k], sb[k]), f"iteration {it}: {k} differs"
        ea.train()
        eb.train()
        assert np.array_equal(ea.get_flat_params(), eb.get_flat_params())
    ea.close()
    eb.close()


def _call_teams(e, env, *, n=4, size=2, sep=0.3, cost=1.0, step0=0, steps=0.0, record=TEAM_START, row=0, hz=0, resume=True,
                teams=True, team_out=True):
    """mobrob_ppo_follow_waypoints_teams straight through ctypes; robot `row` carries `record` and `steps` -> (rc, outputs)"""
    from mobrob_amd import _lib
    P, Kw, St = env.pos_dim, 2, 10
    g = e._goal_env_struct(P, env.mix, 0, False, env.dt, env.extent, 0.3, 5.0, 0.0, 0.0)   # no noise: the robots move alike
    dp, fp, ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    sp = _lib.FollowSpec()
    sp.n_robots, sp.max_waypoints, sp.max_steps, sp.deterministic, sp.seed = n, Kw, St, 1, 1
    wp = np.ones((n, Kw, P), np.float32)
    state, leg, status = np.zeros((n, 6), np.float32), np.zeros(n, np.int32), np.full(n, 77, np.int32)
    rs = _lib.FollowResume()
    rs.step0, rs.leg_steps, rs.state, rs.leg_used, rs.status = step0, 0, state.ctypes.data_as(fp), leg.ctypes.data_as(ip), status.ctypes.data_as(ip)
    tm = _lib.TeamsC()
    tm.team_size, tm.separation, tm.cost, tm.indicator = size, sep, cost, 0
    robot, arrival = np.zeros((n, 4)), np.full((n, Kw), -1, np.int32)
    robot[row, 1] = steps
    to = np.tile(np.array(TEAM_START), (n, 1))
    to[row] = record
    given = to.copy()
    table = np.full((1, 2, 2, 3), 0.3, np.float32)
    hs, hf = _lib.HazardsC(), _lib.HazardFramesC()
    for h in (hs, hf):
        h.n_scenes, h.max_hazards, h.hazards, h.cost, h.indicator = 1, 2, table.ctypes.data_as(fp), 1.0, 0
    hf.n_frames, hf.frame_steps, hf.loop = 2, 3, 0
    hzo = np.tile(np.array([0.0, 0.0, -1.0, np.nan]), (n, 1))
    rc = e.lib.mobrob_ppo_follow_waypoints_teams(
        e._h, C.byref(g), C.byref(sp), C.byref(hs) if hz & 1 else None, C.byref(hf) if hz & 2 else None,
        C.byref(rs) if resume else None, C.byref(tm) if teams else None, wp.ctypes.data_as(fp), None, arrival.ctypes.data_as(ip),
        robot.ctypes.data_as(dp), hzo.ctypes.data_as(dp) if hz else None, to.ctypes.data_as(dp) if team_out else None, None, None)
    return rc, dict(robot=robot, team=to, given=given, status=status, arrival=arrival, hazard=hzo)


@pytest.mark.parametrize("case", [CASES[0], CASES[5], CASES[2]], ids=["fused64", "perstep64", "x3_256"])
def test_invalid_teams_are_refused(case, persistent_env):
    from mobrob_amd import _lib
    name, robot, kw, pe, _ = case
    persistent_env(pe)
    e, _ = _engine(robot, kw)
    env = _env(robot, 4)
    nan = np.nan
    bad = {"size 0": dict(size=0), "size 3": dict(size=3), "size 32": dict(size=32, n=32), "size -2": dict(size=-2),
           "n % size": dict(size=4, n=6), "sep < 0": dict(sep=-0.1), "sep inf": dict(sep=np.inf), "sep nan": dict(sep=nan),
           "cost < 0": dict(cost=-1.0), "cost nan": dict(cost=nan), "no resume": dict(resume=False), "no teams": dict(teams=False),
           "no team_out": dict(team_out=False), "both hazard forms": dict(hz=3),
           "count not whole": dict(steps=5.0, step0=9, record=(0.5, 1.5, 3.0, -0.1, 1.0)),
           "count < 0": dict(steps=5.0, step0=9, record=(0.5, -1.0, 3.0, -0.1, 1.0)),
           "first < -1": dict(steps=5.0, step0=9, record=(0.5, 1.0, -2.0, -0.1, 1.0)),
           "first > step0": dict(steps=5.0, step0=9, record=(0.5, 1.0, 10.0, -0.1, 1.0)),
           "partner itself": dict(steps=5.0, step0=9, record=(0.5, 1.0, 3.0, -0.1, 0.0)),
           "partner of another team": dict(steps=5.0, step0=9, record=(0.5, 1.0, 3.0, -0.1, 2.0)),
           "partner -2": dict(steps=5.0, step0=9, record=(0.5, 1.0, 3.0, -0.1, -2.0)),
           "clearance without steps": dict(steps=0.0, step0=9, record=(0.0, 0.0, -1.0, 0.4, -1.0))}
    for why, b in bad.items():
        rc, o = _call_teams(e, env, **b)
        assert rc == _lib.ERR_INVALID, why
        assert np.array_equal(o["team"], o["given"], equal_nan=True) and np.all(o["status"] == 77), why
    rc, o = _call_teams(e, env, steps=5.0, step0=9, record=(0.5, 1.0, 3.0, -0.1, 1.0))        # a record a call returns: taken
    assert rc in (0, 1) and np.all(o["robot"][1:, 1] == 10) and o["robot"][0, 1] == 15 and np.all(o["status"] != 77)
    assert o["team"][0, 2] == 3 and np.all(o["team"][:, 3] <= -0.3 + 1e-6)                     # all four start on one spot
    for hz in (0, 1, 2):                                                                      # the engine is still usable
        rc, o = _call_teams(e, env, hz=hz)
        assert rc in (0, 1) and np.all(o["team"][:, 1] == 10) and np.all(o["team"][:, 2] == 1), hz
        assert np.array_equal(o["team"][:, 4], [1, 0, 3, 2])
    # the Python surface
    start, wp = np.zeros((4, env.pos_dim), np.float32), np.ones((4, 2, env.pos_dim), np.float32)
    with pytest.raises(ValueError):
        env.follow(e, np.zeros((6, env.pos_dim)), np.ones((6, 2, env.pos_dim)), max_steps=5, teams=Teams(4, 0.3))
    with pytest.raises(TypeError):
        env.follow(e, start, wp, max_steps=5, teams=(2, 0.3))
    plain = env.follow(e, max_steps=5, resume=FollowState(start, wp, None, False, env.pos_dim))
    with pytest.raises(ValueError):
        env.follow(e, max_steps=5, resume=plain["state"], teams=Teams(2, 0.3))
    with pytest.raises(ValueError):
        follow_waypoints(e, env, max_steps=5, state=plain["state"], teams=Teams(2, 0.3))
    team = env.follow(e, start, wp, max_steps=5, teams=Teams(2, 0.3))
    with pytest.raises(ValueError):
        env.follow(e, max_steps=5, resume=team["state"])
    assert np.all(team["steps"] == 5) and team["state"].step0 == 5 and np.all(team["conflict_steps"] == 5)
    e.close()
