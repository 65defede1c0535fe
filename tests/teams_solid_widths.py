"""What tests/test_teams_solid_widths_gpu.py and tests/test_teams_solid_widths_cpu.py share: the shapes, the tracker's weights
without an engine, the scenes, a host stand-in of a solid-team run in the form of a traced device call, and three deliberately
wrong variants of the rule's step.

The host stand-in states the device's observation layout with NumPy's own noise (tests.eval_widths._features), the float64 oracle
actor, goal_rules.goal_propose32 for the proposal and goal_rules.team_block_step (or a variant of it) for the resolve.  Its motion
is not the device's (other noise, float64 actor); its result has the keys tests.test_teams_solid_gpu._teacher reads (trace, path
with path_stride 1, state.state), so the very check the GPU test applies to the device runs on it: the CPU test shows there that
the scenes bite at the new sizes and robots, and that the check rejects a wrong serial order, mates taken where they stood before
the step, and a wrong team base."""
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np

from mobrob_amd.envs.goal_rules import Teams, goal_propose32, team_block, team_block_step, wall_block_velocity
from oracle import ppo_oracle as O
from tests.eval_widths import REACH, _features
from tests.test_teams_solid_gpu import SEP, _scene

T = 64
KW64, KW256 = dict(pi=(64, 64), vf=(64, 64)), dict(pi=(256, 256), vf=(256, 256))
KW_ELU = dict(pi=(32, 32, 32), vf=(32, 32, 32), activation="elu")
KW_SDE = dict(pi=(64, 64), vf=(64, 64), use_sde=True)
DRONE_Z = 0.3                                           # the waypoints of a drone lie this far above its start

# (n, team size, kind) of tests.test_teams_solid_gpu._scene.  n = 24: a tile and a half; n = 40 in teams of 8: the last tile holds
# one team in lanes 0 .. 7; n = 8: a single partial tile
TILE_WIDE_ROBOTS = ["car", "turtlebot3", "drone"]       # DP = 32, 48 and 16 with P = 3, A = 18
TILE_WIDE_SCENES = [(24, 8, "point"), (24, 4, "arena"), (40, 8, "overlap"), (24, 2, "swap")]
TILE_SIZE8_ROBOTS = ["point", "doggo"]
TILE_SIZE8_SCENES = [(24, 8, "point"), (40, 8, "overlap"), (8, 8, "point")]
# the per-step path: n = 80 is two waves (the second with 16 lanes) and two forward() chunks of the reference-shaped engine,
# n = 272 two blocks (the second with 16 threads)
PERSTEP_ROBOTS = ["point", "car"]
PERSTEP_SCENES = [(80, 8, "overlap", 64), (80, 16, "point", 64), (272, 16, "overlap", 32)]
FUSED256_ROBOTS = ["doggo", "car"]
FUSED256_SCENES = [(24, 8, "overlap"), (80, 16, "point")]
ELU_SCENES = [(24, 8, "overlap"), (24, 8, "point")]
SDE_SCENES = [(24, 4, "arena"), (24, 4, "overlap")]
SAMPLED_SCENE = (24, 8, "point")
SPLIT_ROBOTS = ["car", "drone"]
SPLIT_SCENE = (24, 8, "arena", 48)                      # one 48-step call against three 16-step calls


def scene(n, G, kind, P):
    """tests.test_teams_solid_gpu._scene; a drone's waypoints are lifted, so that z has somewhere to go in a blocked step"""
    start, wp, nw, walls = _scene(n, G, kind, P)
    if P == 3:
        wp[:, :, 2] = DRONE_Z
    return start, wp, nw, walls


def tracker_params(robot, kw):
    """the parameters tests.test_teams_solid_gpu._tracker leaves in tests.util._engine(robot, kw), drawn without an engine (the GPU
    test holds the two equal bit for bit), and their like for the other stacks: a go-to-goal actor through every hidden layer of
    the policy (unit i of each layer carries coordinate i; ELU is the identity above 0, so the gain is 1 / 0.1 there), log_std -1
    in whatever shape the stack has, then the tracker's perturbation of every policy weight"""
    from mobrob_amd.engine import param_shapes
    from mobrob_amd.envs.wrapper import ROBOT_DIMS
    from tests.util import _env
    D, A, P = ROBOT_DIMS[robot]
    mix = _env(robot, 16).mix
    act = kw.get("activation", "tanh")
    assert act in ("tanh", "elu") and (act == "elu" or len(kw["pi"]) == 2)
    p = OrderedDict((k, np.zeros(s, np.float32)) for k, s in param_shapes(D, A, kw["pi"], kw["vf"], kw.get("use_sde", False)).items())
    s = 0.1
    for i in range(len(kw["pi"])):
        for j in range(P):
            p[f"mlp_extractor.policy_net.{2 * i}.weight"][j, j] = s if i == 0 else 1.0
    gain = 1.0 / np.tanh(np.tanh(s)) if act == "tanh" else 1.0 / s
    p["action_net.weight"][:, :P] = (gain * np.linalg.pinv(mix.astype(np.float64))).astype(np.float32)
    p["log_std"] = np.full_like(p["log_std"], -1.0)
    rng = np.random.default_rng(5)
    for k, v in p.items():
        if k.startswith(("mlp_extractor.policy_net", "action_net")):
            p[k] = (v + 0.02 * rng.standard_normal(v.shape) / np.sqrt(v.shape[-1])).astype(np.float32)
    return p


# ---- the rule's step and three wrong variants of it: (stand_xy, prop_xy, stepped, teams, walls) -> team_block_step's results ----
def step_reversed(stand, prop, stepped, teams, walls=None):
    """(a) the serial order reversed: the highest team-local index resolves first"""
    n = len(stepped)
    perm = np.arange(n).reshape(-1, teams.size)[:, ::-1].ravel()      # its own inverse
    assert walls is None or walls.scene is None
    return tuple(x[perm] for x in team_block_step(np.asarray(stand)[perm], np.asarray(prop)[perm], np.asarray(stepped)[perm], teams, walls))


def step_prestep(stand, prop, stepped, teams, walls=None):
    """(b) every mate taken where it stood before the step (team_block_step's loop without its publish)"""
    f32 = np.float32
    before = np.array(stand, f32)
    pos, prop, stepped = before.copy(), np.asarray(prop, f32), np.asarray(stepped, bool)
    n, G = len(stepped), teams.size
    assert walls is None or walls.scene is None
    code, flags = np.zeros(n, np.int64), np.zeros((4, n), bool)
    for m in range(G):
        idx = np.arange(m, n, G)
        mates = before.reshape(n // G, G, 2)[:, [j for j in range(G) if j != m]]
        q, c, *fl = team_block(before[idx], prop[idx], mates, teams.separation, None if walls is None else walls.table[0],
                               0.0 if walls is None else walls.radius, None if walls is None else walls.counts[0])
        s = stepped[idx]
        pos[idx] = np.where(s[:, None], q, before[idx])
        code[idx] = np.where(s, c, 0)
        for k in range(4):
            flags[k, idx] = s & fl[k]
    return (pos, code) + tuple(flags)


def step_half_teams(stand, prop, stepped, teams, walls=None):
    """(c) a team of 8 treated as two teams of 4: a wrong team base for members 4 .. 7, and no mate across the halves"""
    assert teams.size == 8
    return team_block_step(stand, prop, stepped, Teams(4, teams.separation, solid=True), walls)


VARIANTS = [("reversed order", step_reversed), ("pre-step mates", step_prestep), ("two teams of four", step_half_teams)]


# ---- the host stand-in ----
def host_run(robot, p, n, G, kind, steps=T, activation="tanh", sampled=0.0, seed=0, step=team_block_step):
    """-> (r, env, teams, walls): r with trace [steps][n][9 + D + A + 4], path [steps + 1][n][P] and state.state [n][6] as a traced
    device call with path_stride = 1 returns them; `sampled`: the standard deviation of Gaussian noise on the actions"""
    from tests.util import _env
    env = _env(robot, n)
    P, D, A = env.pos_dim, env.obs_dim, env.mix.shape[1]
    start, wp, nw, walls = scene(n, G, kind, P)
    teams = Teams(G, SEP, 2.0, solid=True)
    rng = np.random.default_rng(seed)
    pos, vel = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    pos[:, :P] = start
    k = np.zeros(n, int)
    trace, path = np.zeros((steps, n, 9 + D + A + 4), np.float32), np.zeros((steps + 1, n, P), np.float32)
    path[0] = start
    for t in range(steps):
        alive = k < nw
        goal = np.zeros((n, 3), np.float32)
        goal[:, :P] = wp[np.arange(n), np.minimum(k, np.maximum(nw - 1, 0))]
        obs = _features(pos, vel, goal, P, D, rng)
        mean, _ = O.policy_outputs(p, obs, activation=activation)
        act = np.clip(mean + sampled * rng.standard_normal(mean.shape), -1.0, 1.0).astype(np.float32)
        trace[t, alive] = np.concatenate([pos, vel, goal, obs, act, np.ones((n, 4), np.float32)], 1)[alive]
        prop, v = goal_propose32(pos, vel, act, env.mix, env.dt, env.extent, P)
        q, code, *_ = step(pos[:, :2], prop[:, :2], alive, teams, walls)
        pos[alive, :P], vel[alive, :P] = prop[alive], wall_block_velocity(v, code)[alive]
        pos[:, :2] = q
        d = np.linalg.norm(goal[:, :P].astype(np.float64) - pos[:, :P], axis=1)
        k = k + (alive & (d < REACH))
        path[t + 1] = pos[:, :P]
    return dict(trace=trace, path=path, state=SimpleNamespace(state=np.concatenate([pos, vel], 1))), env, teams, walls


def bite(code, inside, by_mate, by_wall, wall_inside, stepped):
    """what a scene's run must show, from _teacher's results -> (steps blocked by a mate, counts of the codes 0 .. 3, inside steps, steps blocked by a wall
    alone)"""
    return (int((by_mate & stepped).sum()), np.bincount(code[stepped], minlength=4), int(inside.sum()), int((by_wall & ~by_mate).sum()))
