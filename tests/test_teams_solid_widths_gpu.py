"""GPU: solid teams at every tile width, in teams of 8, on partial tiles, beyond one wave and one block of the per-step path, and
on every engine that never takes the tile for a team task.

tests/test_teams_solid_gpu.py runs mobrob_ppo_follow_waypoints_teams_solid with point and doggo 2x64 engines at n = 16 and 48 in
teams of 1, 2, 4 and 16, deterministic actions only.  Here, with the same scenes, tracker weights and teacher forcing
(tests.test_teams_solid_gpu: _scene, _tracker, _teacher, _records; the shapes are listed in tests/teams_solid_widths.py):
  the tile     k_goal64_tile<32 | 48 | 16 with P = 3 and A = 18, TeamTask<[WallTask<]SolidTeamFollowTask>> -- car, turtlebot3, drone --
               at n = 24 (a tile and a half) and n = 40 in teams of 8 (the last tile holds one team in lanes 0 .. 7); point and
               doggo in teams of 8 and at n = 8, a single partial tile; car with sampled actions; runs split into calls at a
               partial tile over both bases, with and without solid walls
  per step     2x64 point and car with MOBROB_EVAL_PERSISTENT=0 at n = 80 (two waves, the second with 16 lanes; two forward()
               chunks) in teams of 8 and 16 and at n = 272 (two blocks, the second with 16 threads) in teams of 16
  other stacks fused 2x256 (with nothing set and with both tile256 switches on: the per-step path either way, and the same bits),
               the generic chain (elu 3x32), gSDE (deterministic actions: the entry point refuses a gSDE policy's sampled ones)
Every check is bit for bit against goal_rules (goal_propose32, team_block_step, the folds); the only bound is the existing one of
tests.test_eval_widths_gpu._actor_error for the traced action of a tile run with deterministic actions (a sampled action is not
the actor's mean: the teacher takes it from the trace as it stands).  tests/test_teams_solid_widths_cpu.py shows on the host that
every scene bites and that the teacher check rejects a reversed serial order, mates taken where they stood before the step, and a
team of 8 split into two teams of 4.

Conditions: every scene produces steps blocked by a mate; over the scenes of one engine every code 1 .. 3 occurs and some step is
`inside`; where there are walls some step is blocked by a wall alone.

Measured on the MI355X (printed by the tests): the worst tile action error against the float64 oracle is 9.1e-6 (turtlebot3, n = 40
in teams of 8; bound 1e-5) -- the tracker's head carries a gain of 10 on a hidden layer of magnitude 0.1; the others stay below 4.3e-6."""
import numpy as np
import pytest

from mobrob_amd.envs.goal_rules import Schedule, Teams
from tests import teams_solid_widths as S
from tests.eval_model import trace_fields
from tests.test_eval_tile256_gpu import _engine256
from tests.test_eval_widths_gpu import _actor_error
from tests.test_teams_solid_gpu import SEP, _bits, _records, _teacher, _tracker
from tests.util import _engine, _env, persistent_env  # noqa: F401

pytestmark = pytest.mark.gpu

STATE_FIELDS = ("state", "robot", "arrival", "leg_used", "status", "team", "team_blocked", "sched", "wall", "blocked", "step0")


def _make(robot, kw):
    """the engine with the tracker's weights, held to the ones tests/test_teams_solid_widths_cpu.py examined"""
    want = S.tracker_params(robot, kw)
    if kw is S.KW_ELU:                                    # _tracker's actor reads two hidden layers: the deeper one is set whole
        e, _ = _engine(robot, kw)
        e.set_params(want)
    else:
        e, _ = _engine256(robot, on=False) if kw is S.KW256 else _engine(robot, kw)
        _tracker(e, _env(robot, 16))
    p = e.get_params()
    assert list(p) == list(want) and all(np.array_equal(_bits(p[k]), _bits(want[k])) for k in want)
    return e, p


def _run(e, env, p, what, n, G, kind, steps, persistent, actor, **kw):
    """one scene: the call, the teacher forcing, the records -> (the call's result, _teacher's results)"""
    start, wp, nw, walls = S.scene(n, G, kind, env.pos_dim)
    teams = Teams(G, SEP, 2.0, solid=True)
    r = env.follow(e, start, wp, nw, max_steps=steps, seed=3, path_stride=1, trace=(n, steps), teams=teams, walls=walls, **kw)
    assert r["persistent"] is persistent
    out = _teacher(r, env, teams, walls)
    rec = _records(r, n, teams, walls, *out)
    blocked, codes, inside, wall_only = S.bite(*out)
    print(f"{what} {kind} n={n} G={G}: steps {int(out[-1].sum())} by mate {blocked} codes {codes.tolist()} inside {inside} wall only {wall_only}")
    assert rec[:, 0].sum() > 0 and blocked == rec[:, 0].sum(), (kind, "the rule never bites in this scene")
    if kind == "overlap":
        assert out[1][0].any() and rec[:, 3].sum() > 0
    if actor:
        _actor_error(p, trace_fields(r["trace"], e.D, e.A), out[-1], f"{what} {kind} n={n} G={G}")
    return r, out


def _scenes(e, env, p, what, scenes, persistent, actor, **kw):
    """every scene of a test, and what they must show together"""
    codes, inside, wall_only, with_walls, runs = np.zeros(4, np.int64), 0, 0, False, []
    for sc in scenes:
        n, G, kind = sc[:3]
        r, out = _run(e, env, p, what, n, G, kind, sc[3] if len(sc) > 3 else S.T, persistent, actor, **kw)
        b = S.bite(*out)
        codes, inside, wall_only, with_walls = codes + b[1], inside + b[2], wall_only + b[3], with_walls or kind == "arena"
        runs.append((r, out))
    print(f"{what}: codes {codes.tolist()} inside {inside} walls only {wall_only}")
    assert np.all(codes[1:] > 0) and inside > 0 and (wall_only > 0 or not with_walls)
    return runs


@pytest.mark.parametrize("robot", S.TILE_WIDE_ROBOTS)
def test_tile_at_every_width(robot, persistent_env):
    """k_goal64_tile<32, 48, 16>: the LDS offset of the team's rows follows LayEval64<DP>; drone: the wider state row, the
    second head block, and z through a blocked step"""
    persistent_env(None)
    e, p = _make(robot, S.KW64)
    env = _env(robot, 16)
    runs = _scenes(e, env, p, f"{robot} tile", S.TILE_WIDE_SCENES, True, True)
    if env.pos_dim == 3:                                  # z is no business of a mate or a wall: it moves in the blocked steps too
        for r, out in runs:
            code = out[0]
            rows = np.flatnonzero(code.any(0))
            assert rows.size > 0
            for i in rows:
                t = int(np.flatnonzero(code[:, i])[0])
                assert r["path"][t + 1, i, 2] != r["path"][t, i, 2], (i, t)
    e.close()


@pytest.mark.parametrize("robot", S.TILE_SIZE8_ROBOTS)
def test_tile_teams_of_eight_and_a_partial_tile(robot, persistent_env):
    persistent_env(None)
    e, p = _make(robot, S.KW64)
    _scenes(e, _env(robot, 16), p, f"{robot} tile", S.TILE_SIZE8_SCENES, True, True)
    e.close()


def test_tile_sampled_actions(persistent_env):
    """deterministic=False on the tile: the teacher takes the traced actions, so it applies unchanged"""
    persistent_env(None)
    e, p = _make("car", S.KW64)
    env = _env("car", 16)
    n, G, kind = S.SAMPLED_SCENE
    r, _ = _run(e, env, p, "car tile sampled", n, G, kind, S.T, True, False, deterministic=False)
    det, _ = _run(e, env, p, "car tile", n, G, kind, S.T, True, True)
    assert not np.array_equal(det["path"], r["path"]), "sampled actions should enter"
    e.close()


@pytest.mark.parametrize("robot", S.PERSTEP_ROBOTS)
def test_per_step_path_beyond_a_wave_and_a_block(robot, persistent_env):
    """k_goal_task_step and k_team_step at n = 80 and n = 272: the team's base row in the state rows of the second wave and of the
    second block"""
    persistent_env("0")
    e, p = _make(robot, S.KW64)
    _scenes(e, _env(robot, 16), p, f"{robot} per step", S.PERSTEP_SCENES, False, False)
    e.close()


@pytest.mark.parametrize("robot", S.FUSED256_ROBOTS)
def test_fused_256_stays_on_the_per_step_path(robot, persistent_env):
    """a fused 2x256 engine serves no team task from its tile: with nothing set and with both switches on the call reports the
    per-step path and gives the same bits"""
    persistent_env(None)
    e, p = _make(robot, S.KW256)
    env = _env(robot, 16)
    off = _scenes(e, env, p, f"{robot} 2x256", S.FUSED256_SCENES, False, False)
    e.set_eval_tile256(True)
    e.set_eval_tile256_wide(True)
    for (n, G, kind), (a, _) in zip(S.FUSED256_SCENES, off):
        start, wp, nw, walls = S.scene(n, G, kind, env.pos_dim)
        b = env.follow(e, start, wp, nw, max_steps=S.T, seed=3, path_stride=1, trace=(n, S.T), teams=Teams(G, SEP, 2.0, solid=True), walls=walls)
        assert b["persistent"] is False and set(a) == set(b)
        for k in a:
            if k != "state":
                assert np.array_equal(a[k], b[k], equal_nan=True), (kind, k)
        for f in STATE_FIELDS:
            x, y = getattr(a["state"], f, None), getattr(b["state"], f, None)
            assert (x is None and y is None) or np.array_equal(x, y, equal_nan=True), (kind, f)
    e.close()


def test_generic_chain(persistent_env):
    persistent_env(None)
    e, p = _make("point", S.KW_ELU)
    _scenes(e, _env("point", 16), p, "point elu3x32", S.ELU_SCENES, False, False)
    e.close()


def test_gsde(persistent_env):
    """a gSDE engine: follow_waypoints serves its deterministic actions only, and says so for the others"""
    persistent_env(None)
    e, p = _make("point", S.KW_SDE)
    env = _env("point", 16)
    _scenes(e, env, p, "point sde64", S.SDE_SCENES, False, False)
    n, G, kind = S.SDE_SCENES[0]
    start, wp, nw, walls = S.scene(n, G, kind, env.pos_dim)
    with pytest.raises(ValueError, match="stochastic actions of a use_sde"):
        env.follow(e, start, wp, nw, max_steps=S.T, seed=3, teams=Teams(G, SEP, 2.0, solid=True), walls=walls, deterministic=False)
    e.close()


@pytest.mark.parametrize("robot", S.SPLIT_ROBOTS)
def test_split_runs_at_a_partial_tile(robot, persistent_env):
    """tests/test_teams_solid_gpu.py::test_scheduled_base_and_split_runs at n = 24 in teams of 8: one 48-step call against three
    16-step calls, over ResumeFollowTask (leg_steps) and ScheduledFollowTask (schedule), with and without solid walls"""
    persistent_env(None)
    e, p = _make(robot, S.KW64)
    env = _env(robot, 16)
    n, G, steps = 24, 8, 48
    start, wp, nw, walls = S.scene(n, G, "arena", env.pos_dim)
    teams = Teams(G, SEP, 2.0, solid=True)
    sched = Schedule(np.array([3, 30]) + 2 * (np.arange(n) % 5)[:, None])
    for kw in (dict(leg_steps=20), dict(schedule=sched)):
        for wl in (None, walls):
            one = env.follow(e, start, wp, nw, max_steps=steps, seed=3, path_stride=1, trace=(n, steps), teams=teams, walls=wl, **kw)
            assert one["persistent"] is True
            out = _teacher(one, env, teams, wl)
            rec = _records(one, n, teams, wl, *out)
            assert rec[:, 0].sum() > 0
            if "schedule" in kw:
                assert one["hold_steps"].sum() > 0
            r = env.follow(e, start, wp, nw, max_steps=16, seed=3, teams=teams, walls=wl, **kw)
            for _ in range(2):
                r = env.follow(e, max_steps=16, seed=3, teams=teams, walls=wl, resume=r["state"], **kw)
                assert r["persistent"] is True
            a, b = one["state"], r["state"]
            for f in STATE_FIELDS:
                x, y = getattr(a, f, None), getattr(b, f, None)
                assert (x is None and y is None) or np.array_equal(x, y, equal_nan=True), (sorted(kw), wl is not None, f)
    e.close()
