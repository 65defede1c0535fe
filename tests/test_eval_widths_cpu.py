"""CPU: the inputs of tests/test_eval_widths_gpu.py have the power to fail.

The GPU tests hold k_goal64_tile<16 | 32 | 48 | 64> and k_goal256_tile (8 and 12 layer-1 k-steps) to 1e-5 * max(1, max|want|)
against the float64 oracle on the traced observations.  That is only worth something if a tile that drops or misplaces a k-step
would leave the bound.  Here, for every robot and the exact weights the GPU tests use (tests.eval_widths.host_params: seed 3,
scale 1, nothing rescaled), 60 steps of 24 robots are generated on the host (tests.eval_widths.host_follow: the device's
observation layout, the float64 oracle actor) and the float64 mean is computed with W1 as it is and with W1's columns zeroed from
16, from 32, (turtlebot3) from 40 and from 42, (doggo) from 48 and from 56 upward -- what a tile with a short or misplaced k loop
computes -- and for drone with W3's rows 16 and 17 zeroed, the second head block.  Each corruption that applies to the robot's D
must move the clipped mean by more than 100 x the bound on at least half of the rows.

Measured (fraction of rows moved by more than 100 x the bound, median move), 2x64: car from 16 1.00 / 0.042; turtlebot3 from 16
1.00 / 0.071, from 32 1.00 / 0.039, from 40 0.99 / 0.019, from 42 0.95 / 0.015; doggo from 16 1.00 / 0.14, from 32 1.00 / 0.11, from
48 1.00 / 0.063, from 56 1.00 / 0.022; drone head rows 1.00 / 0.41.  2x256: car 1.00 / 0.045; turtlebot3 1.00 / 0.067, 1.00 / 0.045,
1.00 / 0.021, 0.95 / 0.015.  No seed was changed and no weight scaled.

The second half checks, on the same host motion and with the host rules, that the job, the seeds and the scene builders meet the
conditions the GPU tests assert on their own runs."""
import numpy as np
import pytest

from mobrob_amd.envs.goal_rules import Walls
from oracle import ppo_oracle as O
from tests import eval_widths as W

CUTS = {"car": (16,), "turtlebot3": (16, 32, 40, 42), "doggo": (16, 32, 48, 56), "drone": ()}
CASES = [(r, W.KW64) for r in W.WALL_ROBOTS] + [(r, W.KW256) for r in ("car", "turtlebot3")]
IDS = [f"{r}{kw['pi'][0]}" for r, kw in CASES]


def _moved(p, q, obs):
    """-> (fraction of rows whose clipped mean moves by more than 100 x the GPU bound, the median move)"""
    want = np.clip(O.policy_outputs(p, obs, activation="tanh")[0], -1.0, 1.0)
    got = np.clip(O.policy_outputs(q, obs, activation="tanh")[0], -1.0, 1.0)
    bound = 1e-5 * max(1.0, float(np.max(np.abs(want))))
    move = np.max(np.abs(got - want), axis=1)
    return float(np.mean(move > 100 * bound)), float(np.median(move))


@pytest.mark.parametrize("robot,kw", CASES, ids=IDS)
def test_a_dropped_k_step_leaves_the_bound(robot, kw):
    from mobrob_amd.envs.wrapper import ROBOT_DIMS
    D, A, P = ROBOT_DIMS[robot]
    p = W.host_params(robot, kw)
    start, wp, nw = W.job(P)
    run = W.host_follow(robot, p, start, wp, nw, seed=1)
    obs = run["obs"][run["stepped"]]
    assert obs.shape[1] == D and len(obs) >= W.N * W.T // 2
    assert np.all(np.abs(obs).max(axis=0) > 0), "every feature below D is in use"
    for cut in CUTS[robot]:
        assert cut < D
        q = dict(p)
        q["mlp_extractor.policy_net.0.weight"] = p["mlp_extractor.policy_net.0.weight"].copy()
        q["mlp_extractor.policy_net.0.weight"][:, cut:] = 0
        frac, med = _moved(p, q, obs)
        print(f"{robot} {kw['pi'][0]}: W1 zeroed from column {cut}: {frac:.2f} of {len(obs)} rows move by > 100 x the bound, median {med:.3g}")
        assert frac >= 0.5, (robot, cut, frac)
    if A > 16:
        q = dict(p)
        q["action_net.weight"] = p["action_net.weight"].copy()
        q["action_net.weight"][16:] = 0
        frac, med = _moved(p, q, obs)
        print(f"{robot} {kw['pi'][0]}: W3 rows 16 .. zeroed: {frac:.2f} of {len(obs)} rows move by > 100 x the bound, median {med:.3g}")
        assert frac >= 0.5, (robot, frac)
    assert CUTS[robot] or A > 16


@pytest.mark.parametrize("robot", W.WALL_ROBOTS)
def test_the_job_and_the_scenes_meet_their_conditions_on_host_motion(robot):
    from mobrob_amd.envs.wrapper import ROBOT_DIMS
    P = ROBOT_DIMS[robot][2]
    p = W.host_params(robot, W.KW64)
    start, wp, nw = W.job(P)
    # follow: some robot finishes and some does not; the robot without waypoints never steps
    base = W.host_follow(robot, p, start, wp, nw, seed=1)
    fin = base["reached"] == nw
    assert np.any(fin & (nw > 0)) and np.any(~fin) and base["ran"][W.NO_WAYPOINTS] == 0 and nw[W.ONE_WAYPOINT] == 1
    assert np.sum(base["ran"] == W.T) >= 9, "robots that run the whole call: the scenes are built on them"
    # evaluation: some episode truncates (time limit 40 < 60 steps)
    ev = W.host_evaluate(robot, p, seed=2)
    assert ev["truncations"] > 0
    # a schedule with staggered releases: some hold steps, also of robots that go on afterwards
    held = W.host_follow(robot, p, start, wp, nw, seed=1, rel=W.release())
    assert np.any(held["holds"] > 0) and np.any(held["holds"] == 0) and held["ran"][W.NO_WAYPOINTS] == 0
    # solid walls from the wall-free run: the three chosen robots are blocked, some robot never is (same noise: same motion up
    # to the first block), and drone's z passes through
    boxes, rows = W.solid_scene(base["ran"], base["path"], base["stepped"])
    assert len(set(rows)) == 3 and any(i >= 16 for i in rows) and any(i < 16 for i in rows)
    solid = W.host_follow(robot, p, start, wp, nw, seed=1, walls=Walls(boxes, radius=W.RADIUS_SOLID, solid=True))
    blocked = (solid["code"] != 0).sum(0)
    assert np.all(blocked[rows] > 0) and np.sum(blocked > 0) >= 3 and np.any((blocked == 0) & (solid["ran"] > 0))
    free = blocked == 0
    assert np.array_equal(solid["path"][:, free], base["path"][:, free])
    if P == 3:
        assert np.any(solid["path"][1:, rows, 2] != solid["path"][:-1, rows, 2])
