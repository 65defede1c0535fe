"""The goal task's rules as array functions over a batch of robots.

What the reference evaluates one robot at a time inside `EnvWrapper` (/root/reference/src/mobrob/envs/wrapper.py:
reward :137-154, termination :156-171, lazy reset :173-201, reach test :203-207) is stated here once, over `[n]` /
`[n, p]` arrays, so that every consumer applies literally the same rules: the single-robot `EnvWrapper` (n = 1),
the worker processes of `ShmVecEnv`, and the tests that compare the C (`csrc/host_env.c`) and device
(`csrc/kernels_env.h`) implementations against them.

The reward is stated on DISTANCES: a robot carries the distance to its goal measured at the end of its previous
step (`NaN` = nothing measured yet), and the step reward is the decrease of that distance -- the same number as
`|goal - prev_pos| - |goal - pos|`, because the goal only changes inside `reset`, which re-measures.
"""
from __future__ import annotations

import numpy as np

REACH_RADIUS = 0.3   # wrapper.py:203
GOAL_BONUS = 5.0     # wrapper.py:151-152


def goal_distance(goal, pos):
    """Euclidean distance robot -> goal, row-wise: [n, p], [n, p] -> [n] (float64)."""
    delta = np.asarray(goal, np.float64) - np.asarray(pos, np.float64)
    return np.sqrt(np.einsum("...i,...i->...", delta, delta))


def inside_goal(dist, radius=REACH_RADIUS):
    """Strictly inside the reach radius."""
    return np.asarray(dist) < radius


def progress_reward(prev_dist, dist, radius=REACH_RADIUS, bonus=GOAL_BONUS):
    """Decrease of the goal distance since the previous step (zero where no previous distance exists) plus the
    reach bonus -> (reward [n] float64, reached [n] bool)."""
    prev_dist, dist = np.asarray(prev_dist, np.float64), np.asarray(dist, np.float64)
    gain = np.where(np.isnan(prev_dist), 0.0, prev_dist - dist)
    hit = inside_goal(dist, radius)
    return gain + bonus * hit, hit


def episode_over(reached, terminate_on_goal):
    """`terminated` of the gymnasium 5-tuple: only goal arrival ends an episode, and only if asked to."""
    return np.logical_and(bool(terminate_on_goal), reached)


def must_respawn(ever_reset, reached):
    """Lazy reset: a robot is put back to a sampled start pose at its first reset and whenever the episode ended
    WITHOUT reaching the goal (time limit: it may be stuck); one that has just arrived keeps its pose and only
    receives a new goal."""
    return np.logical_or(np.logical_not(ever_reset), np.logical_not(reached))


# ---- hazards: the reference Engine's `constrain_hazards` cost (engine.py: config :230-244, rule :1329-1345, dist_xy
# :1037-1043, info :1432).  Hazards are circles on the floor (vertical cylinders): only x and y count, for every robot.
HAZARDS_SIZE = 0.3       # hazards_size
HAZARDS_COST = 1.0       # hazards_cost
HAZARDS_MAX = 1024       # hazards per scene the device path takes


def hazard_cost(pos, hazards, coef=HAZARDS_COST, indicator=True):
    """Per-step hazard cost at post-step positions: pos [..., p] (p = 1..3; a missing y is 0), hazards [M, 3] rows
    (x, y, radius) or [..., M, 3] per position -> (cost [...], clearance [...]) in float64.

    cost = sum over hazards with d <= r of coef * (r - d), d = |pos_xy - h_xy|; with `indicator` cost = (cost > 0).
    A robot exactly on a boundary (d == r) is charged 0 by that hazard.  clearance = min (d - r), +inf without hazards."""
    pos = np.asarray(pos, np.float64)
    xy = np.zeros(pos.shape[:-1] + (2,))
    xy[..., : min(pos.shape[-1], 2)] = pos[..., :2]
    hz = np.asarray(hazards, np.float64).reshape(np.shape(hazards)[:-1] + (3,)) if np.size(hazards) else np.zeros((0, 3))
    d = np.sqrt(np.sum(np.square(xy[..., None, :] - hz[..., :2]), axis=-1))   # [..., M]
    r = hz[..., 2]
    cost = float(coef) * np.sum(np.where(d <= r, r - d, 0.0), axis=-1)
    clear = np.min(d - r, axis=-1, initial=np.inf)
    if indicator:
        cost = (cost > 0.0).astype(np.float64)
    return cost, clear


class Hazards:
    """A hazard layout: `locations` [M, 2] (one scene) or [S, M, 2] (scenes), `size` a radius for all or per hazard ([M] /
    [S, M]), `counts` [S] hazards in use per scene (None: all M), `scene` [n] scene of each robot (None: S must be 1),
    `cost` (hazards_cost) and `indicator` (constrain_indicator).  Checked on construction (ValueError)."""

    def __init__(self, locations, size=HAZARDS_SIZE, cost=HAZARDS_COST, indicator=True, counts=None, scene=None):
        loc = np.asarray(locations, np.float64)
        if loc.size == 0 and loc.ndim < 2:
            loc = loc.reshape(0, 2)
        if loc.ndim == 2:
            loc = loc[None]
        if loc.ndim != 3 or loc.shape[2] != 2:
            raise ValueError(f"hazard locations must be [M, 2] or [S, M, 2], got shape {np.shape(locations)}")
        S, M = loc.shape[:2]
        if S < 1:
            raise ValueError("hazards need at least one scene")
        if M > HAZARDS_MAX:
            raise ValueError(f"at most {HAZARDS_MAX} hazards per scene, got {M}")
        rad = np.asarray(size, np.float64)
        if rad.shape not in ((), (M,), (S, M)):
            raise ValueError(f"hazard size must be a scalar, [{M}] or [{S}, {M}], got shape {rad.shape}")
        rad = np.broadcast_to(rad, (S, M))
        if not (np.all(np.isfinite(loc)) and np.all(np.isfinite(rad))):
            raise ValueError("hazard locations and sizes must be finite")
        if np.any(rad < 0):
            raise ValueError("hazard sizes must be >= 0")
        cost = float(cost)
        if not np.isfinite(cost) or cost < 0:
            raise ValueError(f"hazard cost must be finite and >= 0, got {cost}")
        if counts is None:
            cnt = np.full(S, M, np.int32)
        else:
            cnt = np.asarray(counts)
            if cnt.shape != (S,) or not np.issubdtype(cnt.dtype, np.integer) or np.any(cnt < 0) or np.any(cnt > M):
                raise ValueError(f"hazard counts must be {S} integers in 0 .. {M}")
            cnt = cnt.astype(np.int32)
        if scene is None:
            if S != 1:
                raise ValueError(f"{S} hazard scenes need a scene index per robot")
            sc = None
        else:
            sc = np.asarray(scene)
            if sc.ndim != 1 or not np.issubdtype(sc.dtype, np.integer) or np.any(sc < 0) or np.any(sc >= S):
                raise ValueError(f"hazard scene indices must be integers in 0 .. {S - 1}")
            sc = sc.astype(np.int32)
        self.table = np.ascontiguousarray(np.concatenate([loc, rad[..., None]], axis=-1), np.float32)   # [S, M, 3]
        self.counts, self.scene, self.cost, self.indicator = cnt, sc, cost, bool(indicator)

    @property
    def n_scenes(self):
        return self.table.shape[0]

    @property
    def max_hazards(self):
        return self.table.shape[1]

    def rows(self, robot=0):
        """[m, 3] (x, y, radius) float64 of the hazards robot `robot` sees (the float32 values the device uses)."""
        s = 0 if self.scene is None else int(self.scene[robot])
        return self.table[s, : self.counts[s]].astype(np.float64)

    def check_robots(self, n):
        if self.scene is not None and self.scene.shape != (n,):
            raise ValueError(f"hazard scene must have {n} entries, one per robot, got {self.scene.shape[0]}")
