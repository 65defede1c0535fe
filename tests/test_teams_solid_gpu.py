"""GPU: solid teams on the device (mobrob_ppo_follow_waypoints_teams_solid; Teams(..., solid=True) on PPOEngine.follow_waypoints and
DeviceGoalVecEnv.follow): point and doggo 2x64 engines with fixed random weights, n = 16 (one tile of k_goal64_tile) and n = 48
(three tiles: a wrong team base shows), 64 steps, teams of 2, 4, 16 and 1, on the tile and forced onto the per-step path.  The
weights are fixed random ones around a go-to-goal actor (_tracker): with purely random weights the robots of a team drift side by
side and never meet.

Teacher forcing: from the call's own trace, for every step goal_rules.goal_propose32 of the traced (position, velocity, action) and
then goal_rules.team_block_step in the rule's serial order must give the next position and velocity, the path record and the
carried state bit for bit; the records are then folded from the rule's codes.  The scenes start the mates a little more than the
separation apart (or inside each other) and send them through each other, so the rule bites: every scene must produce blocked steps, and
every (robot, path) every code and the inside case."""
import numpy as np
import pytest

from mobrob_amd.envs.goal_rules import (BLOCKED_START, TEAM_BLOCKED_START, TEAM_START, WALL_START, Hazards, MovingHazards, Schedule,
                                        Teams, Walls, goal_propose32, team_block_fold, team_block_step, team_fold,
                                        wall_block_velocity, wall_blocked_fold, wall_fold)
from mobrob_amd.waypoints import FollowState, follow_waypoints, team_blocked_result
from tests.util import _engine, _env, _go_to_goal_params, persistent_env  # noqa: F401

pytestmark = pytest.mark.gpu

T, K, SEP, RADIUS = 64, 2, 0.25, 0.05
NET = dict(pi=(64, 64), vf=(64, 64))
CASES = [("point", None, True), ("point", "0", False), ("doggo", None, True), ("doggo", "0", False)]
CASE_IDS = ["point-tile", "point-perstep", "doggo-tile", "doggo-perstep"]
SCENES = [(16, 2, "swap"), (48, 4, "point"), (48, 16, "overlap"), (16, 16, "inactive"), (48, 4, "arena"), (48, 2, "overlap")]
TEAM_KEYS = tuple(team_blocked_result(FollowState(np.zeros((2, 2)), np.zeros((2, 1, 2)), teams=Teams(2, SEP, solid=True))))


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _scene(n, G, kind, P):
    """-> start [n][P], waypoints [n][K][P], counts [n], walls or None.  Members on a small grid around their team's centre:
    a little more than the separation apart (overlap: well inside each other), the centres 0.45 apart on a grid of their own."""
    rng = np.random.default_rng(7 * n + G)
    side = int(np.ceil(np.sqrt(G)))
    spacing = (0.4 if kind == "overlap" else 1.06) * SEP
    local = (np.stack([np.arange(G) % side, np.arange(G) // side], 1) - 0.5 * (side - 1)) * spacing
    teams = n // G
    cols = int(np.ceil(np.sqrt(teams)))
    centre = (np.stack([np.arange(teams) % cols, np.arange(teams) // cols], 1) - 0.5 * (cols - 1)) * 0.45
    start = np.zeros((n, P))
    start[:, :2] = (centre[:, None] + local[None]).reshape(n, 2) + rng.uniform(-0.004, 0.004, (n, 2))
    wp = np.zeros((n, K, P))
    nw = np.full(n, K, np.int32)
    home = np.repeat(centre, G, 0)
    xy = start[:, :2]
    if kind == "swap":                                    # mates change places: each one's waypoint lies beyond its partner
        partner = xy.reshape(teams, G, 2)[:, ::-1].reshape(n, 2)
        wp[:, 0, :2], wp[:, 1, :2] = xy + 4.0 * (partner - xy), xy
    elif kind == "overlap":                               # apart, then across the middle to the far side, all of them
        out = 0.7 * (xy - home) / np.linalg.norm(xy - home, axis=1, keepdims=True)
        wp[:, 0, :2], wp[:, 1, :2] = home + out, home - out
    elif kind == "inactive":                              # member 1 never steps: an obstacle from step 0, the others are sent to it
        wp[:, 0, :2], wp[:, 1, :2] = np.repeat(xy[1::G], G, 0), home + (0.5, -0.4)
        nw[np.arange(1, n, G)] = 0
    else:                                                 # point, arena: the whole team to one point, and back to another
        wp[:, 0, :2], wp[:, 1, :2] = home + (0.5, 0.4), home
    walls = None
    if kind == "arena":                                   # the enclosure and two boxes between the teams: the combined resolve
        boxes = np.concatenate([Walls.enclosure(), [[0.23, 0.0, 0.02, 0.6], [-0.3, 0.25, 0.4, 0.02]]])
        walls = Walls(boxes, radius=RADIUS, cost=1.5, indicator=False, solid=True)
    return start.astype(np.float32), wp.astype(np.float32), nw, walls


def _tracker(e, env):
    """fixed random weights around a go-to-goal actor: the robots head for their waypoints (so the scenes make mates meet), with
    every unit of the net carrying a value"""
    _go_to_goal_params(e, env)
    rng = np.random.default_rng(5)
    p = e.get_params()
    for k, v in p.items():
        if k.startswith(("mlp_extractor.policy_net", "action_net")):
            p[k] = (v + 0.02 * rng.standard_normal(v.shape) / np.sqrt(v.shape[-1])).astype(np.float32)
    e.set_params(p)


def _setup(case, persistent_env, n):
    robot, pe, expect = case
    persistent_env(pe)
    e, _ = _engine(robot, NET)
    env = _env(robot, n)
    _tracker(e, env)
    return e, env, expect


def _teacher(r, env, teams, walls=None):
    """every step of a traced call with path_stride = 1 checked bit for bit against the rule -> (code, inside, by_mate, by_wall,
    wall_inside, stepped), each [T][n]"""
    P, A = env.pos_dim, env.mix.shape[1]
    tr, path = r["trace"], r["path"]
    steps, n = tr.shape[:2]
    D = tr.shape[2] - 9 - A - 4
    stepped = np.any(tr != 0, axis=2)
    pos, vel, act = tr[..., 0:3], tr[..., 3:6], tr[..., 9 + D:9 + D + A]
    prop, v = goal_propose32(pos, vel, act, env.mix, env.dt, env.extent, P)
    code = np.zeros((steps, n), np.int64)
    inside, by_mate, by_wall, wall_inside = (np.zeros((steps, n), bool) for _ in range(4))
    last_vel = np.zeros((n, P), np.float32)
    for t in range(steps):
        s = stepped[t]
        stand = path[t, :, :2]                            # where everybody stands before step t (a robot that does not step: there)
        assert np.array_equal(_bits(stand[s]), _bits(pos[t, s, :2])), (t, "pre-step position")
        q, code[t], inside[t], by_mate[t], by_wall[t], wall_inside[t] = team_block_step(stand, prop[t, :, :2], s, teams, walls)
        want = path[t].copy()
        want[s] = prop[t, s]
        want[:, :2] = q
        bad = np.flatnonzero(np.any(_bits(path[t + 1]) != _bits(want), axis=1))
        assert bad.size == 0, (t, bad.tolist(), "position after the step")
        want_vel = wall_block_velocity(v[t], code[t])
        if t + 1 < steps:
            nxt = s & stepped[t + 1]
            assert np.array_equal(_bits(tr[t + 1, nxt, 3:3 + P]), _bits(want_vel[nxt])), (t, "velocity")
        last_vel[s] = want_vel[s]
    st = r["state"].state
    ran = stepped.any(0)
    assert np.array_equal(_bits(st[:, :P]), _bits(path[-1])) and np.array_equal(_bits(st[ran, 3:3 + P]), _bits(last_vel[ran]))
    return code, inside, by_mate, by_wall, wall_inside, stepped


def _records(r, n, teams, walls, code, inside, by_mate, by_wall, wall_inside, stepped, step0=0):
    st = r["state"]
    want = team_block_fold(np.tile(TEAM_BLOCKED_START, (n, 1)), code, inside, by_mate, stepped, step0)
    assert np.array_equal(st.team_blocked, want)
    for k, v in team_blocked_result(st).items():
        assert np.array_equal(r[k], v), k
    post = r["path"][1:, :, :2]
    assert np.array_equal(st.team, team_fold(np.tile(np.array(TEAM_START), (n, 1)), post, stepped, teams, step0), equal_nan=True)
    if walls is not None:
        assert np.array_equal(st.blocked, wall_blocked_fold(np.tile(BLOCKED_START, (n, 1)), np.where(by_wall, code, 0), wall_inside, stepped, step0))
        assert np.array_equal(st.wall, wall_fold(np.tile(WALL_START, (n, 1)), r["path"][:-1, :, :2], post, stepped, walls, step0), equal_nan=True)
    else:
        assert st.blocked is None and st.wall is None
    return want


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_teacher_forcing(case, persistent_env):
    e, env, expect_persistent = _setup(case, persistent_env, 48)
    seen = np.zeros(4, np.int64)
    n_inside = n_wall_only = n_both = 0
    for n, G, kind in SCENES:
        start, wp, nw, walls = _scene(n, G, kind, env.pos_dim)
        teams = Teams(G, SEP, 2.0, solid=True)
        r = env.follow(e, start, wp, nw, max_steps=T, seed=3, path_stride=1, trace=(n, T), teams=teams, walls=walls)
        assert r["persistent"] == expect_persistent
        code, inside, by_mate, by_wall, wall_inside, stepped = _teacher(r, env, teams, walls)
        rec = _records(r, n, teams, walls, code, inside, by_mate, by_wall, wall_inside, stepped)
        counts = np.bincount(code[stepped], minlength=4)
        print(f"{case[0]} {kind} n={n} G={G}: steps {int(stepped.sum())} codes {counts.tolist()} inside {int(inside.sum())} "
              f"by mate {int(by_mate.sum())} by wall {int(by_wall.sum())}")
        assert rec[:, 0].sum() > 0, (kind, "the rule never bites in this scene")
        if kind == "overlap":
            assert inside[0].any() and rec[:, 3].sum() > 0
        if kind == "inactive":
            assert not stepped[:, 1::G].any() and np.all(r["path"][:, 1::G] == r["path"][0, 1::G])
        # the guarantee on the device's own output: a team none of whose members was ever inside a mate keeps its distance
        clean = np.repeat(rec[:, 3].reshape(-1, G).sum(1) == 0, G) & (r["steps"] > 0)
        assert np.all(r["min_team_clearance"][clean] > -1e-6)
        if walls is not None:
            free = r["wall_inside_steps"] == 0
            assert np.all(r["crossing_steps"][free] == 0) and np.all(r["min_wall_clearance"][free & (r["steps"] > 0)] > -1e-6)
        seen += counts
        n_inside += int(inside.sum())
        n_wall_only += int((by_wall & ~by_mate).sum())
        n_both += int((by_wall & by_mate).sum())
    print(f"{case[0]}: codes {seen.tolist()} inside {n_inside} walls only {n_wall_only} walls and mates {n_both}")
    assert np.all(seen[1:] > 0) and n_inside > 0 and n_wall_only > 0
    e.close()


@pytest.mark.parametrize("case", CASES[:2], ids=CASE_IDS[:2])
def test_scheduled_base_and_split_runs(case, persistent_env):
    e, env, _ = _setup(case, persistent_env, 48)
    n, G = 48, 4
    start, wp, nw, walls = _scene(n, G, "arena", env.pos_dim)
    teams = Teams(G, SEP, 2.0, solid=True)
    sched = Schedule(np.array([3, 30]) + 2 * (np.arange(n) % 5)[:, None])
    for kw in (dict(leg_steps=20), dict(schedule=sched), dict(schedule=sched, leg_steps=25)):
        for wl in (None, walls):
            one = env.follow(e, start, wp, nw, max_steps=T, seed=3, path_stride=1, trace=(n, T), teams=teams, walls=wl, **kw)
            out = _teacher(one, env, teams, wl)
            rec = _records(one, n, teams, wl, *out)
            assert rec[:, 0].sum() > 0
            if "schedule" in kw:
                assert one["hold_steps"].sum() > 0
            r = env.follow(e, start, wp, nw, max_steps=16, seed=3, teams=teams, walls=wl, **kw)
            for _ in range(3):
                r = env.follow(e, max_steps=16, seed=3, teams=teams, walls=wl, resume=r["state"], **kw)
            a, b = one["state"], r["state"]
            for f in ("state", "robot", "arrival", "leg_used", "status", "team", "team_blocked", "sched", "wall", "blocked", "step0"):
                x, y = getattr(a, f, None), getattr(b, f, None)
                assert (x is None and y is None) or np.array_equal(x, y, equal_nan=True), (sorted(kw), wl is not None, f)
    e.close()


@pytest.mark.parametrize("case", CASES[:2], ids=CASE_IDS[:2])
def test_observational_calls_keep_their_bits(case, persistent_env):
    e, env, _ = _setup(case, persistent_env, 48)
    n = 48
    start, wp, nw, walls = _scene(n, 4, "arena", env.pos_dim)

    def same(a, b, why, skip=TEAM_KEYS):
        for k in a:
            if k not in ("state", "persistent") and k not in skip:
                assert np.array_equal(a[k], b[k], equal_nan=True), (why, k)
        for f in ("state", "robot", "arrival", "leg_used", "status", "team", "wall", "blocked"):
            x, y = getattr(a["state"], f, None), getattr(b["state"], f, None)
            assert (x is None and y is None) or np.array_equal(x, y, equal_nan=True), (why, f)
    for wl in (None, walls):
        run = dict(max_steps=T, seed=3, path_stride=1, trace=(n, T), walls=wl)
        # solid=False is today's call; a team of one has no mate: the solid call gives the bits of the call without `solid`
        plain = env.follow(e, start, wp, nw, teams=Teams(4, SEP, 2.0), **run)
        same(plain, env.follow(e, start, wp, nw, teams=Teams(4, SEP, 2.0, solid=False), **run), "solid=False", skip=())
        assert plain["state"].team_blocked is None and "team_blocked_steps" not in plain
        alone = env.follow(e, start, wp, nw, teams=Teams(1, SEP, 2.0), **run)
        solo = env.follow(e, start, wp, nw, teams=Teams(1, SEP, 2.0, solid=True), **run)
        same(alone, solo, "teams of one")
        assert np.array_equal(solo["state"].team_blocked, np.tile(TEAM_BLOCKED_START, (n, 1)))
        # mates that never come near each other: nothing to block
        far = start.copy()
        far[:, :2] = (np.stack([np.arange(n) % 7, np.arange(n) // 7], 1) - 3.0) * 0.33
        lazy = wp.copy()
        lazy[:, :, :2] = far[:, None, :2] + 0.01
        a = env.follow(e, far, lazy, nw, teams=Teams(4, 0.05, 2.0), **run)
        b = env.follow(e, far, lazy, nw, teams=Teams(4, 0.05, 2.0, solid=True), **run)
        if np.all(a["min_team_clearance"] > 0.05):        # (no pair within a step of the other's square: the rule cannot bite)
            same(a, b, "far mates")
            assert np.array_equal(b["state"].team_blocked, np.tile(TEAM_BLOCKED_START, (n, 1)))
    e.close()


def test_refusals(persistent_env):
    e, env, _ = _setup(CASES[0], persistent_env, 16)
    n = 16
    start, wp, nw, walls = _scene(n, 4, "arena", env.pos_dim)
    solid = Teams(4, SEP, solid=True)
    moving = MovingHazards.circling(np.array([[0.0, 0.0]]), 0.3, [0.4], 4, 2.0, frame_steps=7, loop=True)
    static = Hazards(np.array([[0.0, 0.0]]), [0.4])
    for call in (lambda **kw: env.follow(e, start, wp, nw, max_steps=5, seed=3, **kw),
                 lambda **kw: follow_waypoints(e, env, start, wp, nw, max_steps=5, seed=3, **kw)):
        with pytest.raises(ValueError, match=r"Teams\(solid=True\) does not run with MovingHazards"):
            call(teams=solid, hazards=moving)
        with pytest.raises(ValueError, match=r"Teams\(solid=True\) does not run with static hazards"):
            call(teams=solid, hazards=static)
        with pytest.raises(ValueError, match=r"Teams\(solid=True\) does not run with observational walls"):
            call(teams=solid, walls=Walls(walls.table[0], radius=RADIUS))
    with pytest.raises(ValueError, match="solid teams in every call or in none"):
        env.follow(e, max_steps=5, seed=3, teams=solid, resume=FollowState(start, wp, nw, pos_dim=env.pos_dim, teams=True))
    with pytest.raises(ValueError, match="solid teams in every call or in none"):
        env.follow(e, max_steps=5, seed=3, teams=Teams(4, SEP), resume=FollowState(start, wp, nw, pos_dim=env.pos_dim, teams=solid))
    with pytest.raises(ValueError, match="not a multiple of team_size|do not split into teams"):
        env.follow(e, start[:6], wp[:6], nw[:6], max_steps=5, seed=3, teams=solid)
    for col, v in ((0, -1), (0, 1), (1, 3), (2, 1), (3, 9)):   # a carried record no call returns: refused by the entry point
        st = FollowState(start, wp, nw, pos_dim=env.pos_dim, teams=solid)
        st.team_blocked[2, col] = v
        with pytest.raises(ValueError, match="follow: solid teams: carried team-blocked record of robot 2"):
            env.follow(e, max_steps=5, seed=3, teams=solid, resume=st)
    ok = env.follow(e, start, wp, nw, max_steps=5, seed=3, teams=solid, walls=walls)      # the engine is as usable as before
    assert np.all(ok["steps"][nw > 0] == 5) and "team_blocked_steps" in ok and "wall_blocked_steps" in ok
    e.close()
