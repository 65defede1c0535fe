"""What tests/test_eval_widths_gpu.py and tests/test_eval_widths_cpu.py share: the shapes, the engines' weights without an engine,
the job, the scenes built from a run, and a host stand-in of the device goal environment under the float64 oracle actor.

The host stand-in states the device's observation layout (csrc/kernels_env.h goal_features: unit vector to the goal, velocity,
position, then obs_noise * N(0, 1) in every further feature) with NumPy's own noise, tests/eval_model.goal_advance for the step
and the host rules of goal_rules for holds and solid walls.  Its motion is not the device's (other noise, float64 actor); it is
what the CPU test checks the seeds, jobs and scenes on before the GPU sees them."""
from collections import OrderedDict

import numpy as np

from mobrob_amd.envs.goal_rules import Schedule, wall_block, wall_block_velocity
from oracle import ppo_oracle as O
from tests.eval_model import goal_advance

N, K, T, TL = 24, 2, 60, 40                             # robots (a full 16-robot tile and a half one), waypoints, steps, time limit
ROBOTS = ["car", "turtlebot3", "drone"]                 # tile widths 32, 48, 16 (drone: A = 18, the second head block; P = 3)
WALL_ROBOTS = ROBOTS + ["doggo"]                        # 64
KW64, KW256 = dict(pi=(64, 64), vf=(64, 64)), dict(pi=(256, 256), vf=(256, 256))
ENGINE_SEED, EVAL_SEED, FOLLOW_SEED = 3, 9, 3
NOISE, REACH = 0.1, 0.3
NO_WAYPOINTS, ONE_WAYPOINT = 5, 19                      # robots with n_waypoints = 0 and 1
RADIUS_WALL, RADIUS_SOLID = 0.12, 0.04
FAR = [[50.0, 50.0, 1.0, 1.0], [-40.0, 30.0, 0.5, 2.0], [0.0, -60.0, 3.0, 0.1]]


def host_params(robot, kw, seed=ENGINE_SEED, scale=1.0):
    """the parameters tests.util._engine(robot, kw, seed=seed, scale=scale) sets, drawn without an engine (the GPU test holds the
    two equal bit for bit)"""
    from mobrob_amd.engine import param_shapes
    from mobrob_amd.envs.wrapper import ROBOT_DIMS
    D, A, _ = ROBOT_DIMS[robot]
    rng = np.random.default_rng(seed)
    p = OrderedDict()
    for k, shape in param_shapes(D, A, kw["pi"], kw["vf"]).items():
        if k == "log_std":
            p[k] = np.full(shape, -0.5, np.float32)
        elif len(shape) == 2:
            p[k] = (scale * rng.standard_normal(shape) / np.sqrt(shape[1])).astype(np.float32)
        else:
            p[k] = (0.1 * rng.standard_normal(shape)).astype(np.float32)
    return p


def job(P, seed=11):
    """-> start [N][P], waypoints [N][K][P], counts [N].  Every third robot's waypoints lie 2 and 4 cm from its start (inside the
    reach radius: it arrives on consecutive steps and finishes); the others' lie 1 to 2 m away, out of a random actor's way.  Robot
    NO_WAYPOINTS never steps, robot ONE_WAYPOINT has a single (far) waypoint."""
    rng = np.random.default_rng(seed)
    start = rng.uniform(-1.5, 1.5, (N, P))
    u = rng.standard_normal((N, K, P))
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    near = start[:, None, :] + 0.02 * (np.arange(K)[None, :, None] + 1) * u[:, :1]
    far = np.clip(start[:, None, :] + rng.uniform(1.0, 2.0, (N, K, 1)) * u, -2.5, 2.5)
    wp = np.where((np.arange(N) % 3 == 0)[:, None, None], near, far)
    nw = np.full(N, K, np.int32)
    nw[NO_WAYPOINTS], nw[ONE_WAYPOINT] = 0, 1
    return start.astype(np.float32), wp.astype(np.float32), nw


def release():
    """staggered release steps [N][K]: waypoint 0 at 0, 3, 6, 9 by robot, and waypoint 1 twenty steps later -- but together with
    waypoint 0 for every third robot, whose waypoints lie next to its start: held for twenty steps under a random actor it would
    drift out of reach, and no robot of the scheduled runs would finish"""
    rel = np.array([0, 20]) + 3 * (np.arange(N) % 4)[:, None]
    rel[::3, 1] = rel[::3, 0]
    return rel.astype(np.int32)


# ---- scenes from a traced run with path_stride = 1 (its `steps`, `path` [T + 1][N][P] and who stepped [T][N]) ----
def segments(path, stepped):
    xy = np.zeros(path.shape[:2] + (2,), np.float32)
    xy[..., :2] = path[..., :2]
    return xy[:-1], xy[1:], stepped


def runners(steps, path, t, away):
    """the robots that run all T steps and stand more than `away` from their start (in x, y) before step t, farthest first"""
    d = np.linalg.norm(path[t, :, :2].astype(np.float64) - path[0, :, :2], axis=1)
    rows = [int(i) for i in np.argsort(-d, kind="stable") if steps[i] == T and d[i] > away]
    return rows


def spread(rows, k):
    """k of `rows`, the first of them from the half tile (robots 16 ..) and the second from the full one where there are such"""
    half, full = [i for i in rows if i >= 16], [i for i in rows if i < 16]
    out = half[:1] + full[:1]
    out += [i for i in rows if i not in out]
    assert len(out) >= k, (rows, k)
    return out[:k]


def thin_box(pre, post, i, t):
    """a box of half-thickness 1e-4 across the midpoint of robot i's step t, thin across the larger component of the motion"""
    a, p = pre[t, i].astype(np.float64), post[t, i].astype(np.float64)
    d = np.abs(p - a)
    return [*(0.5 * (a + p)), *((1e-4, 0.02) if d[0] >= d[1] else (0.02, 1e-4))]


SOLID_STEP = 30


def solid_scene(steps, path, stepped):
    """-> (boxes [6][4], the three robots that get a thin box across their step SOLID_STEP).  They stand more than 0.15 from their
    start by then, so the start lies outside the box inflated by RADIUS_SOLID and the robot must be blocked on its way in."""
    pre, post, _ = segments(path, stepped)
    rows = spread(runners(steps, path, SOLID_STEP, 0.15), 3)
    return np.array([thin_box(pre, post, i, SOLID_STEP) for i in rows] + FAR), rows


# ---- the host stand-in ----
def _features(pos, vel, goal, P, D, rng):
    n = len(pos)
    obs = NOISE * rng.standard_normal((n, D))
    d = np.linalg.norm(goal[:, :P].astype(np.float64) - pos[:, :P], axis=1, keepdims=True) + 1e-6
    obs[:, :P] = (goal[:, :P] - pos[:, :P]) / d
    obs[:, P:2 * P], obs[:, 2 * P:3 * P] = vel[:, :P], pos[:, :P]
    return obs.astype(np.float32)


def _act(p, obs):
    mean, _ = O.policy_outputs(p, obs, activation="tanh")
    return np.clip(mean, -1.0, 1.0).astype(np.float32)


def host_follow(robot, p, start, wp, nw, steps=T, seed=0, rel=None, walls=None):
    """-> dict(obs [steps][n][D], stepped [steps][n], path [steps + 1][n][P], reached [n], steps [n], holds [n], code [steps][n])"""
    from tests.util import _env
    env = _env(robot, len(start))
    P, D = env.pos_dim, env.obs_dim
    n = len(start)
    rng = np.random.default_rng(seed)
    pos, vel = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    pos[:, :P] = start
    k, alive = np.zeros(n, int), nw > 0
    out = dict(obs=np.zeros((steps, n, D), np.float32), stepped=np.zeros((steps, n), bool), path=np.zeros((steps + 1, n, P), np.float32),
               holds=np.zeros(n, int), code=np.zeros((steps, n), int), ran=np.zeros(n, int))
    out["path"][0] = start
    for t in range(steps):
        hold = (Schedule.holding(rel, nw, k, t) & alive) if rel is not None else np.zeros(n, bool)
        goal = np.zeros((n, 3), np.float32)
        g = Schedule.goal(rel, start, wp, nw, k, t) if rel is not None else wp[np.arange(n), np.minimum(k, np.maximum(nw - 1, 0))]
        goal[:, :P] = np.nan_to_num(g)
        obs = _features(pos, vel, goal, P, D, rng)
        act = _act(p, obs)
        pos2, vel2, _, reached = goal_advance(pos, vel, goal, act, env.mix, P, env.dt, env.extent)
        if walls is not None:
            for i in np.flatnonzero(alive):
                q, c, _ = wall_block(pos[i, :2], pos2[i, :2], walls.rows(i), walls.radius)
                pos2[i, :2], vel2[i] = q, wall_block_velocity(vel2[i], c)
                out["code"][t, i] = int(c)
            d = np.linalg.norm(goal[:, :P].astype(np.float64) - pos2, axis=1)
            reached = d < REACH
        out["obs"][t], out["stepped"][t] = np.where(alive[:, None], obs, 0), alive
        pos[alive, :P], vel[alive, :P] = pos2[alive], vel2[alive]
        out["ran"] += alive
        out["holds"] += hold
        k = k + (alive & ~hold & reached)
        alive = alive & (k < nw)
        out["path"][t + 1] = pos[:, :P]
    out["reached"] = k
    return out


def host_evaluate(robot, p, n=N, steps=T, tl=TL, seed=0):
    """-> dict(obs [steps][n][D], pos [steps][n][2] before each step, truncations, goals)"""
    from tests.util import _env
    env = _env(robot, n, tl=tl)
    P, D = env.pos_dim, env.obs_dim
    rng = np.random.default_rng(seed)
    pos, vel, goal = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    pos[:, :P], goal[:, :P] = rng.uniform(-env.extent / 2, env.extent / 2, (n, P)), rng.uniform(-env.extent, env.extent, (n, P))
    age = np.zeros(n, int)
    out = dict(obs=np.zeros((steps, n, D), np.float32), pos=np.zeros((steps, n, 2), np.float32), truncations=0, goals=0)
    for t in range(steps):
        obs = _features(pos, vel, goal, P, D, rng)
        out["obs"][t], out["pos"][t] = obs, pos[:, :2]
        pos2, vel2, _, reached = goal_advance(pos, vel, goal, _act(p, obs), env.mix, P, env.dt, env.extent)
        pos[:, :P], vel[:, :P] = pos2, vel2
        age += 1
        tr = ~reached & (age >= tl)
        goal[reached, :P] = rng.uniform(-env.extent, env.extent, (int(reached.sum()), P))
        pos[tr, :P], vel[tr] = rng.uniform(-env.extent / 2, env.extent / 2, (int(tr.sum()), P)), 0
        age[reached | tr] = 0
        out["truncations"] += int(tr.sum())
        out["goals"] += int(reached.sum())
    return out
