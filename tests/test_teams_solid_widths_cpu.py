"""What tests/test_teams_solid_widths_gpu.py rests on, shown without a GPU (NumPy and the float64 oracle only).

1. The tracker's weights drawn on the host (tests.teams_solid_widths.tracker_params) are the ones tests.test_teams_solid_gpu._tracker
   leaves in an engine.
2. Every scene of the GPU test bites under the host stand-in (tests.teams_solid_widths.host_run), with margin: at least 5 steps
   blocked by a mate per scene; over the scenes of one engine every code 1 .. 3, some step `inside` and, where there are walls, some
   step blocked by a wall alone.  The stand-in's own run passes the teacher check the GPU test applies to the device.
3. That check discriminates: a run produced by the serial order reversed, by every mate taken where it stood before the step, or
   by a team of 8 treated as two teams of 4 is rejected by tests.test_teams_solid_gpu._teacher in the teams-of-8 scenes of every
   robot -- a kernel with a wrong order, a missing fence or a wrong team base would fail the GPU test."""
from collections import OrderedDict
from functools import lru_cache

import numpy as np
import pytest

from mobrob_amd.envs.goal_rules import TEAM_BLOCKED_START, team_block_fold
from tests import teams_solid_widths as S
from tests.test_teams_solid_gpu import _bits, _teacher, _tracker

SAMPLED_STD = float(np.exp(-1.0))                       # the tracker's log_std is -1
# (id, robot, engine, scenes, noise on the actions, the conditions over the scenes together)
GROUPS = ([(f"{r}-tile", r, S.KW64, S.TILE_WIDE_SCENES, 0.0, True) for r in S.TILE_WIDE_ROBOTS]
          + [(f"{r}-tile", r, S.KW64, S.TILE_SIZE8_SCENES, 0.0, True) for r in S.TILE_SIZE8_ROBOTS]
          + [(f"{r}-perstep", r, S.KW64, S.PERSTEP_SCENES, 0.0, True) for r in S.PERSTEP_ROBOTS]
          + [(f"{r}-256", r, S.KW256, S.FUSED256_SCENES, 0.0, True) for r in S.FUSED256_ROBOTS]
          + [("elu3x32", "point", S.KW_ELU, S.ELU_SCENES, 0.0, True), ("sde64", "point", S.KW_SDE, S.SDE_SCENES, 0.0, True),
             ("car-sampled", "car", S.KW64, [S.SAMPLED_SCENE], SAMPLED_STD, False)]
          + [(f"{r}-split", r, S.KW64, [S.SPLIT_SCENE], 0.0, False) for r in S.SPLIT_ROBOTS])
SIZE8_ROBOTS = S.TILE_WIDE_ROBOTS + S.TILE_SIZE8_ROBOTS
SIZE8_SCENES = [(24, 8, "point"), (40, 8, "overlap")]   # of TILE_WIDE_SCENES and TILE_SIZE8_SCENES both
VARIANT_STEPS = 32


class _Params:
    """what _tracker needs of an engine"""

    def __init__(self, robot, kw):
        from mobrob_amd.engine import param_shapes
        from mobrob_amd.envs.wrapper import ROBOT_DIMS
        D, A, _ = ROBOT_DIMS[robot]
        self.p = OrderedDict((k, np.ones(s, np.float32)) for k, s in param_shapes(D, A, kw["pi"], kw["vf"], kw.get("use_sde", False)).items())

    def get_params(self):
        return OrderedDict((k, v.copy()) for k, v in self.p.items())

    def set_params(self, d):
        self.p = OrderedDict((k, np.asarray(d[k], np.float32).copy()) for k in self.p)


@pytest.mark.parametrize("robot,kw", [("car", S.KW64), ("drone", S.KW64), ("doggo", S.KW256), ("point", S.KW_SDE)],
                         ids=["car64", "drone64", "doggo256", "point-sde"])
def test_tracker_params_are_the_trackers(robot, kw):
    from tests.util import _env
    e = _Params(robot, kw)
    _tracker(e, _env(robot, 16))
    want = S.tracker_params(robot, kw)
    assert list(e.p) == list(want) and all(np.array_equal(_bits(e.p[k]), _bits(want[k])) for k in want)


@lru_cache(maxsize=None)
def _params(robot, name):
    return S.tracker_params(robot, {"64": S.KW64, "256": S.KW256, "elu": S.KW_ELU, "sde": S.KW_SDE}[name])


def _name(kw):
    return "256" if kw is S.KW256 else "elu" if kw is S.KW_ELU else "sde" if kw is S.KW_SDE else "64"


@pytest.mark.parametrize("group", GROUPS, ids=[g[0] for g in GROUPS])
def test_scenes_bite_on_the_host(group):
    _, robot, kw, scenes, noise, together = group
    codes, inside, wall_only, with_walls = np.zeros(4, np.int64), 0, 0, False
    for sc in scenes:
        n, G, kind = sc[:3]
        r, env, teams, walls = S.host_run(robot, _params(robot, _name(kw)), n, G, kind, sc[3] if len(sc) > 3 else S.T,
                                          kw.get("activation", "tanh"), noise)
        out = _teacher(r, env, teams, walls)              # the stand-in's own run passes the check
        code, ins, by_mate, _, _, stepped = out
        b = S.bite(*out)
        rec = team_block_fold(np.tile(TEAM_BLOCKED_START, (n, 1)), code, ins, by_mate, stepped)
        print(f"{group[0]} {sc}: steps {int(stepped.sum())} by mate {b[0]} codes {b[1].tolist()} inside {b[2]} wall only {b[3]}")
        assert rec[:, 0].sum() == b[0] and b[0] >= 5, (sc, "the rule does not bite in this scene")
        if kind == "overlap":
            assert ins[0].any()
        if env.pos_dim == 3:                              # what the GPU test asks of a drone: z moves in the first blocked step
            for i in np.flatnonzero(code.any(0)):
                t = int(np.flatnonzero(code[:, i])[0])
                assert r["path"][t + 1, i, 2] != r["path"][t, i, 2], (sc, i, t)
        codes, inside, wall_only, with_walls = codes + b[1], inside + b[2], wall_only + b[3], with_walls or walls is not None
    if together:
        assert np.all(codes[1:] >= 5) and inside >= 5 and (wall_only >= 5 or not with_walls), (codes, inside, wall_only)


@pytest.mark.parametrize("robot", SIZE8_ROBOTS)
def test_the_teacher_rejects_a_wrong_rule(robot):
    p = _params(robot, "64")
    rejected = {name: [] for name, _ in S.VARIANTS}
    for n, G, kind in SIZE8_SCENES:
        good, env, teams, walls = S.host_run(robot, p, n, G, kind, VARIANT_STEPS)
        _teacher(good, env, teams, walls)
        for name, step in S.VARIANTS:
            bad, *_ = S.host_run(robot, p, n, G, kind, VARIANT_STEPS, step=step)
            if np.array_equal(bad["path"], good["path"]):   # the variant never differed from the rule in this scene
                continue
            with pytest.raises(AssertionError) as err:
                _teacher(bad, env, teams, walls)
            rejected[name].append((kind, str(err.value)[:60]))
    print(robot, rejected)
    assert all(len(v) > 0 for v in rejected.values()), rejected
